"""The input side of the engine (stem.hip: stem_conv_kernel in its four forms at 32 and 64 channels, stem_mfma_kernel,
maxpool3x3s2_kernel, subsample2_kernel) against tests/stem_ref.py at valid edges, element by element.

Every engine runs phase 0 of td_engine_forward_phase (the trunk only: no proposal or detection selection, so a 1 x 1 valid
image is a legal input) on batches whose bytes outside each image's valid rectangle are sentinels: seeded random bytes
(uint8) or NaN (float). Asserted per case:
  * `stem` inside the float64 bound of tests/stem_ref.py at EVERY element (the MFMA engine against its model and against
    the truth), with at least 30 % of the reference outputs inside the valid area positive;
  * `pool` = the 3 x 3 / stride 2 / pad 1 maximum of the engine's own `stem`, bit for bit;
  * `p6` = p5[:, ::2, ::2], bit for bit (96 x 160 gives p5 = 3 x 5: the odd-size subsample).
Geometries (tests/stem_ref.GEOMETRIES): mixed valid sizes with a degenerate image; valid edges on, before and after the tile
seams; and, for the MFMA engine, 896 tiles against its 768 resident blocks (the persistent walk and its prefetch).
Schedule: the TD_PHASE_STEM pre-phase followed by phase 0, and an engine that runs the backbone in sub-batches of 2 (ragged
last pass of a batch of 3), leave the same `stem` and `pool` bits as one plain phase 0.
The fp16 engine has no 32-channel trunk (its convolutions take 64-channel k-chunks), so the two 32-channel fp16 forms of
stem_conv_kernel and the fp16 pool behind them run through TD_PHASE_STEM alone, which is the stem and the pool.
The worst err / bound per engine is printed at the end of the module (pytest -s)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import stem_ref as sr
from tests.test_engine_gpu import TOL_ACT
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu

SD_ARGS = {"half": dict(depth=50, seed=3, width_div=2), "full": dict(depth=50, seed=5)}
# name → (state dict, precision, environment around Engine(...), stem channels, the MFMA stem on uint8 input)
ENGINES = {
    "fp32_c32": ("half", "fp32", {}, 32, False),
    "fp16_c32": ("half", "fp16", {}, 32, False),
    "fp32_c64": ("full", "fp32", {}, 64, False),
    "fp16_c64_mfma": ("full", "fp16", {}, 64, True),
    "fp16_c64_valu": ("full", "fp16", {"TD_STEM_MFMA": "0"}, 64, False),
    "fp32_c32_subbatch2": ("half", "fp32", {"TD_BACKBONE_SUBBATCH": "2"}, 32, False),
    "fp16_c64_mfma_subbatch2": ("full", "fp16", {"TD_BACKBONE_SUBBATCH": "2"}, 64, True),
}
MFMA_RESIDENT_BLOCKS = 768          # stem_launch: 256 CUs x 3 blocks
TOL_FP16_TRUNK = 8e-3               # tests/test_engine_fp16_gpu.py::test_fp16_trunk_close_to_fp32


@functools.lru_cache(maxsize=None)
def state_dict(key):
    return make_synthetic_state_dict(**SD_ARGS[key])


@functools.lru_cache(maxsize=None)
def params(key):
    return sr.stem_params(state_dict(key))


@functools.lru_cache(maxsize=None)
def batch_and_reference(sd_key, geometry, fmt):
    """(batch, Reference, MfmaReference or None) of one case: computed once, shared by every test, never modified."""
    torch.set_num_threads(8)
    B, Hp, Wp, valid = sr.GEOMETRIES[geometry]
    batch = sr.make_batch(fmt, B, Hp, Wp, valid, seed=100 + 2 * sorted(sr.GEOMETRIES).index(geometry) + fmt)
    pix, mask = sr.pixels(batch, valid)
    ref = sr.reference(params(sd_key), pix, mask)
    assert ref.positive >= sr.MIN_POSITIVE, (sd_key, geometry, fmt, ref.positive)        # teeth, on the reference alone
    mref = sr.mfma_reference(params(sd_key), pix, mask) if fmt == sr.INPUT_U8_HWC and sd_key == "full" else None
    batch.setflags(write=False)
    return batch, ref, mref


@pytest.fixture(scope="module")
def engine():
    """Engines by name, built on first use, closed when the module is done."""
    from treedetection_amd.engine import Engine
    made = {}

    def get(name):
        if name not in made:
            sd_key, prec, env, _, _ = ENGINES[name]
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[name] = Engine(state_dict(sd_key), precision=prec)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def worst():
    """Worst err / bound per engine (and reference), printed once at the end."""
    w = {}
    yield w
    print("\n[stem] worst err / bound per engine: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(w.items())))


STEM_ONLY = ("fp16_c32",)           # engines whose trunk cannot run: the stem pre-phase alone


def run_trunk(eng, batch, fmt, valid, names=("stem", "pool", "p5", "p6"), prephase=False, stem_only=False):
    """Phase 0 (optionally behind the stem pre-phase, or that pre-phase alone) on one batch → the named engine tensors on
    the host."""
    from treedetection_amd.engine import PHASE_STEM
    x = torch.from_numpy(np.array(batch)).cuda()
    B = x.shape[0]
    Hp, Wp = (x.shape[2], x.shape[3]) if fmt == sr.INPUT_F32_CHW else (x.shape[1], x.shape[2])
    out = eng.alloc_outputs(B, Hp, Wp, paste=False)
    st = torch.cuda.current_stream()
    if prephase or stem_only:
        eng.forward_phase(PHASE_STEM, st, x, fmt, valid, valid, out)
        if not stem_only:
            eng.forward_phase(0, st)
    else:
        eng.forward_phase(0, st, x, fmt, valid, valid, out)
    torch.cuda.synchronize()
    return {n: eng.tensor(n).cpu() for n in names}


def check_stem(name, geometry, fmt, stem, worst):
    """`stem` [B, Ho, Wo, C] of engine `name` against the float64 bound(s), every element."""
    sd_key, prec, _, C, mfma = ENGINES[name]
    B, Hp, Wp, _ = sr.GEOMETRIES[geometry]
    _, ref, mref = batch_and_reference(sd_key, geometry, fmt)
    assert tuple(stem.shape) == (B, Hp // 2, Wp // 2, C)
    assert stem.dtype == (torch.float16 if prec == "fp16" else torch.float32)
    got = sr.nchw(stem)
    label = name.replace("_subbatch2", "")
    if mfma and fmt == sr.INPUT_U8_HWC:
        for tag, want, bound in (("model", mref.model, mref.model_bound), ("truth", ref.y64, mref.truth_bound)):
            ok, ratio, where = sr.worst_ratio(got, want, bound)
            print(f"\n[stem] {name} {geometry} uint8 against the {tag}: worst err / bound {ratio:.3g} at {where}")
            worst[f"{label}/{tag}"] = max(worst.get(f"{label}/{tag}", 0.0), ratio)
            assert ok, (name, geometry, tag, ratio, where)
        return
    ok, ratio, where = sr.worst_ratio(got, ref.y64, ref.bound16 if prec == "fp16" else ref.bound)
    print(f"\n[stem] {name} {geometry} {'uint8' if fmt == sr.INPUT_U8_HWC else 'float'}: worst err / bound {ratio:.3g} at {where}")
    worst[label] = max(worst.get(label, 0.0), ratio)
    assert ok, (name, geometry, fmt, ratio, where)


def check_moves(got):
    """pool and p6 are pure data movement of the engine's own stem and p5: bit for bit."""
    stem, pool = got["stem"].numpy(), got["pool"].numpy()
    assert sr.same_bits(pool, sr.maxpool_ref(stem)), "pool differs from the 3x3/s2/p1 maximum of the engine's stem"
    if "p6" in got:
        p5, p6 = got["p5"].numpy(), got["p6"].numpy()
        assert sr.same_bits(p6, np.ascontiguousarray(p5[:, ::2, ::2])), "p6 differs from p5[:, ::2, ::2]"


CASES = [(e, g) for e in ("fp32_c32", "fp16_c32", "fp32_c64", "fp16_c64_valu", "fp16_c64_mfma") for g in ("mixed", "seams", "seams2", "seams3")]
CASES.append(("fp16_c64_mfma", "walk"))


@pytest.mark.parametrize("name,geometry", CASES)
def test_stem_pool_p6_against_float64(name, geometry, engine, worst):
    B, Hp, Wp, valid = sr.GEOMETRIES[geometry]
    if geometry == "walk":
        tiles = -(-(Wp // 2) // 16) * -(-(Hp // 2) // 8) * B
        assert tiles > MFMA_RESIDENT_BLOCKS, tiles             # some blocks walk a second tile through the prefetch
    if geometry.startswith("seams"):
        assert all(v in sr.SEAM for hw in valid for v in hw) and (Hp // 32, Wp // 32) == (3, 5)
    mfma = ENGINES[name][4]
    for fmt in ((sr.INPUT_U8_HWC,) if mfma else (sr.INPUT_U8_HWC, sr.INPUT_F32_CHW)):     # (the MFMA engine's float form is fp16_c64_valu's)
        batch, _, _ = batch_and_reference(ENGINES[name][0], geometry, fmt)
        only = name in STEM_ONLY
        got = run_trunk(engine(name), batch, fmt, valid, names=("stem", "pool") if only else ("stem", "pool", "p5", "p6"), stem_only=only)
        check_stem(name, geometry, fmt, got["stem"], worst)
        check_moves(got)
        if geometry.startswith("seams") and not only:
            assert tuple(got["p5"].shape[1:3]) == (3, 5) and tuple(got["p6"].shape[1:3]) == (2, 3)


@pytest.mark.parametrize("name", ["fp32_c32", "fp16_c64_mfma"])
def test_stem_prephase_leaves_the_same_bits(name, engine):
    """TD_PHASE_STEM followed by phase 0 of the same batch = phase 0 alone, for stem and pool bit for bit."""
    _, _, _, valid = sr.GEOMETRIES["mixed"]
    batch, _, _ = batch_and_reference(ENGINES[name][0], "mixed", sr.INPUT_U8_HWC)
    eng = engine(name)
    plain = run_trunk(eng, batch, sr.INPUT_U8_HWC, valid, names=("stem", "pool"))
    # another batch in between, so that the buffers do not simply still hold the plain run's result
    other, _, _ = batch_and_reference(ENGINES[name][0], "mixed", sr.INPUT_F32_CHW)
    between = run_trunk(eng, other, sr.INPUT_F32_CHW, valid, names=("stem",))
    assert not sr.same_bits(between["stem"].numpy(), plain["stem"].numpy())
    staged = run_trunk(eng, batch, sr.INPUT_U8_HWC, valid, names=("stem", "pool"), prephase=True)
    for k in ("stem", "pool"):
        assert sr.same_bits(staged[k].numpy(), plain[k].numpy()), k


@pytest.mark.parametrize("name", ["fp32_c32", "fp16_c64_mfma"])
def test_backbone_subbatches_leave_the_same_stem_and_pool(name, engine, worst):
    """TD_BACKBONE_SUBBATCH=2 on a batch of 3: passes of 2 and 1 images with the image pointer, the valid-size table and
    the stem / pool buffers offset. stem and pool: the whole-batch engine's bits, and stem inside the float64 bound. res5
    and p2 may differ in summation order (the tile choice follows the row count): within TOL_ACT of the whole-batch engine
    for fp32; for fp16, where a different order moves an fp16 rounding now and then, within the fp16 trunk's 8e-3 — an
    offset that is wrong moves them by their own magnitude."""
    _, _, _, valid = sr.GEOMETRIES["mixed"]
    names = ("stem", "pool", "res5", "p2")
    for fmt in (sr.INPUT_U8_HWC, sr.INPUT_F32_CHW):
        batch, _, _ = batch_and_reference(ENGINES[name][0], "mixed", fmt)
        whole = run_trunk(engine(name), batch, fmt, valid, names=names)
        sub = run_trunk(engine(name + "_subbatch2"), batch, fmt, valid, names=names)
        for k in ("stem", "pool"):
            assert sr.same_bits(sub[k].numpy(), whole[k].numpy()), (k, fmt)
        check_stem(name + "_subbatch2", "mixed", fmt, sub["stem"], worst)
        tol = TOL_FP16_TRUNK if ENGINES[name][1] == "fp16" else TOL_ACT
        for k in ("res5", "p2"):
            a, b = sub[k].double(), whole[k].double()
            assert float(b.abs().max()) > 0 and bool(torch.isfinite(a).all())
            rel = float((a - b).abs().max() / b.abs().max())
            print(f"\n[stem] {name} sub-batches of 2, {k}: max |diff| / max {rel:.3g}")
            assert rel <= tol, (k, fmt, rel)
