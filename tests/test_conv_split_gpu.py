"""The split-bf16 contraction tiles (conv_split.hip, tile ids 34 - 36) through td_conv2d_nhwc against the float64 reference of
tests/conv_ref.py — its bound and RMS_MAX unchanged —, bit equality among the ids, the refusals, and the engine with the split
rule on (the default) against itself and against TD_F32_SPLIT=0."""
import os

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests.conv_split_cases import NS, SHORT_K, SPLIT_IDS

pytestmark = pytest.mark.gpu

# k-chunk counts (32 floats): 1, 2, NS = 3 (one full turn of the loop), NS + 1 and at least 4 NS, with every remainder of the
# count by NS (the loop's tail) — the short-K shapes (2, 1, 4, 8 chunks) and the first two below (3, 12); then the long accumulation
# (392 chunks, a 37-row FC) and several column blocks with the last one partial (1056 = 4 x 256 + 32 = 8 x 128 + 32; 32 chunks)
CASES = SHORT_K + [
    (cr.Conv("s96x40", 32 * NS, 40, 1, 1, 0, 9, 11), 1),
    (cr.Conv("s384x72", 32 * 4 * NS, 72, 1, 1, 0, 7, 9), 2),
    (cr.Conv("fc12544x64", 12544, 64, 1, 1, 0, 1, 1), 37),
    (cr.Conv("s1024x1056.res", 1024, 1056, 1, 1, 0, 9, 7, res=1), 2),
]
_CHUNKS = {L.Cin // 32 for L, _ in CASES}
assert _CHUNKS >= {1, 2, NS, NS + 1, 4 * NS} and {c % NS for c in _CHUNKS} == set(range(NS))


@pytest.mark.parametrize("L,B", CASES, ids=[L.name for L, _ in CASES])
def test_split_tiles_against_float64_and_each_other(L, B):
    seed = 101 + L.Cin
    inp = cr.make_inputs(L, False, B, "cuda", seed)
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed))
    y0 = cr.new_output(L, inp)
    cr.launch(L, inp, y0, 0)
    v0 = cr.check(L, y0, ref)
    print(f"\n[{L.name} B={B}] M={B * L.Ho * L.Wo} K={L.K} N={L.Cout}\n  tile  0: err/bound {v0.err_over_bound:.3g}  RMS {v0.rms:.3g}")
    assert v0.ok, v0.why
    first = None
    for cfg in SPLIT_IDS:
        y = cr.new_output(L, inp)
        cr.launch(L, inp, y, cfg, strict=True)
        v = cr.check(L, y, ref)
        print(f"  tile {cfg}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        assert v.ok, f"tile {cfg}: {v.why}"
        if first is None:
            first = y
        else:
            assert torch.equal(y.t.view(y.ity), first.t.view(first.ity)), f"tile {cfg} differs from tile {SPLIT_IDS[0]}"


@pytest.mark.parametrize("cfg", SPLIT_IDS)
def test_split_tiles_are_refused_on_3x3_and_fp16(cfg):
    for L, fp16 in ((cr.Conv("r3x3", 64, 64, 3, 1, 1, 8, 8), False), (cr.Conv("r16", 64, 64, 1, 1, 0, 8, 8), True)):
        inp = cr.make_inputs(L, fp16, 1, "cuda", 3)
        with pytest.raises(Exception, match=f"tile_cfg {cfg} cannot run"):
            cr.launch(L, inp, cr.new_output(L, inp), cfg, strict=True)


def _engine_outputs(sd, tiles, split):
    from treedetection_amd.engine import Engine, INPUT_U8_HWC
    if split is not None:
        os.environ["TD_F32_SPLIT"] = split
    try:
        eng = Engine(sd, device=0, precision="fp32")
        images, hw_valid, hw_out = eng.preprocess_tiles_u8(tiles)
        o = eng.alloc_outputs(2, 600, 600, paste=False)
        eng.forward_raw(images, INPUT_U8_HWC, hw_valid, hw_out, o)
        eng.forward_raw(images, INPUT_U8_HWC, hw_valid, hw_out, o)          # second pass: measured tile choices in use
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().copy() for k, v in o.items()}
        eng.close()
    finally:
        os.environ.pop("TD_F32_SPLIT", None)
    return out


def _same_detections(a, b):
    return all(np.array_equal(a[k][i][:int(a["count"][i])], b[k][i][:int(a["count"][i])]) for k in ("boxes", "scores", "mask_probs") for i in range(2))


def _within_golden_tolerances(a, off, what):
    print(f"\ncounts: {what} {a['count'].tolist()}, fp32 tiles {off['count'].tolist()}")
    assert np.array_equal(a["count"], off["count"])
    for k, tol in (("scores", 1e-4), ("boxes", 1e-2), ("mask_probs", 1e-3)):
        d = max(float(np.abs(a[k][i][:int(a["count"][i])] - off[k][i][:int(a["count"][i])]).max()) for i in range(2))
        print(f"max |d {k}| = {d:.3g} (tolerance {tol})")
        assert d <= tol, k


def test_engine_with_the_split_rule_repeats_itself_and_agrees_with_the_fp32_tiles():
    """Two default engines (each measures its own tile choice among the split ids): bit-equal outputs. The default against
    TD_F32_SPLIT=0 (every layer on its fp32 tiles): the same detections, within tests/test_golden_gpu.py's tolerances — and NOT
    bit for bit: the split tiles round differently, so equal bits would mean that fc1 / fc2 fell back to their fp32 tiles. Every
    class of the rule at once (TD_F32_SPLIT=31: the FPN laterals and the 1x1 layers of res3 - res5 too, off by default) against
    the fp32 tiles likewise, and different from the default."""
    from treedetection_amd.synth import make_tile
    from treedetection_amd.weights import make_synthetic_state_dict
    sd = make_synthetic_state_dict(50, seed=0)
    tiles = [torch.from_numpy(make_tile(i, 600)[0]).cuda() for i in range(2)]
    a, b, off = _engine_outputs(sd, tiles, None), _engine_outputs(sd, tiles, None), _engine_outputs(sd, tiles, "0")
    assert a["count"].sum() > 0 and np.array_equal(a["count"], b["count"])
    assert _same_detections(a, b)
    _within_golden_tolerances(a, off, "split")
    assert not _same_detections(a, off), "the default engine equals TD_F32_SPLIT=0 bit for bit: fc1 / fc2 did not run a split tile"
    every = _engine_outputs(sd, tiles, "31")
    _within_golden_tolerances(every, off, "every class")
    assert not _same_detections(every, off) and not _same_detections(every, a), "TD_F32_SPLIT=31 changed no layer beyond the box head"
