"""Every direct conv tile with the two launch properties only the mask head uses — a row count read from device memory
(ConvArgs::m_dyn / m_mul) and the pixel-shuffle store of the deconvolution (out_mode 1) — through td_conv2d_rows_nhwc, against
the float64 reference of tests/conv_ref.py.

B = 8 reserved RoIs of 14 x 14 at the mask head's production widths, fp32 and fp16; counts 0, 1, 3, 7, 8 and 9 RoIs with
rows_mul = 196 (3 RoIs = 588 rows: a partial block at every block height from 32 to 256; 9 must clamp to 8). The input's RoIs at
and past the count hold quiet NaN, y and its guards hold the sentinel. For every id of SWEEP_IDS under strict selection: the
accepted set is the one conv_ref.tile_runs states and contains every tuner candidate; ALL live rows and channels pass the fp64
bound and the RMS criterion (conv_ref's constants, unchanged); no live output is non-finite; every element at or past the count
still holds the sentinel; the live rows equal, bit for bit, the same rows of the same id's static launch over all 8 RoIs; the
stated bit-identical families equal tile 0; at count 0 nothing is written."""
import functools

import pytest
import torch

from tests import conv_ref as cr

pytestmark = pytest.mark.gpu

B = 8
COUNTS = [0, 1, 3, 7, 8, 9]
LAYERS = {
    "mask.conv": cr.Conv("mask.conv", 256, 256, 3, 1, 1, 14, 14, scale=False),
    "mask.deconv": cr.Conv("mask.deconv", 256, 1024, 1, 1, 0, 14, 14, scale=False, out_mode=1),
}
BIT_IDENTICAL_TO_0 = {17, 23, 24, 25, 26, 27, 29, 30, 33}      # as in tests/test_conv_shapes_gpu.py: tile 0's k order and epilogue
WORST = {}                                                     # (layer, dtype) -> [worst err/bound, worst RMS]


def _bits(g, n=None):
    t = g.t if n is None else g.t[:n]
    return t.reshape(-1).view(g.ity)


def _run_ids(L, inp, ref, count_t, live_rows, tag):
    """Force every sweep id on one launch; -> (accepted ids, failures, outputs by id)."""
    accepted, fails, ys = [], [], {}
    for cfg in cr.SWEEP_IDS:
        y = cr.new_output(L, inp)
        try:
            cr.launch(L, inp, y, cfg, strict=True, count=count_t, rows_entry=True)
        except Exception as e:                                          # a refusal must name the id and say why
            if f"tile_cfg {cfg} cannot run" not in str(e):
                fails.append(f"tile {cfg}: unexpected error {e}")
            elif not (y.guards_intact() and y.pattern_count() == y.n):
                fails.append(f"tile {cfg}: refused, but y was written")
            continue
        accepted.append(cfg)
        v = cr.check(L, y, ref, live_rows=live_rows)
        w = WORST.setdefault((L.name, str(y.t.dtype).replace("torch.", "")), [0.0, 0.0])
        w[0], w[1] = max(w[0], v.err_over_bound), max(w[1], v.rms)
        print(f"  [{tag}] tile {cfg:2d}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        if not v.ok:
            fails.append(f"tile {cfg}: {v.why}")
        ys[cfg] = y
        if cfg in BIT_IDENTICAL_TO_0 and 0 in ys and not torch.equal(_bits(y), _bits(ys[0])):
            fails.append(f"tile {cfg}: {int((_bits(y) != _bits(ys[0])).sum())} elements differ from tile 0 (stated bit-identical)")
    return accepted, fails, ys


@functools.lru_cache(maxsize=None)
def _static(name, fp16):
    """Seeded inputs with all 8 RoIs valid, the float64 reference of EVERY row (once per layer and precision), and every
    id's static launch (rows_dyn = NULL) over them."""
    L = LAYERS[name]
    inp = cr.make_inputs(L, fp16, B, "cuda", seed=1000 + 2 * list(LAYERS).index(name) + int(fp16))
    ref = cr.reference(L, inp, torch.arange(B * L.Ho * L.Wo))
    print(f"\n[{name} {'fp16' if fp16 else 'fp32'} static]")
    accepted, fails, ys = _run_ids(L, inp, ref, None, None, "static")
    return L, inp, ref, accepted, fails, ys


def _with_dead_rois(L, inp, live):
    """A copy of the inputs whose RoIs at and past `live` hold quiet NaN (inside its own NaN-guarded allocation)."""
    x = cr.Guarded(tuple(inp["x"].t.shape), inp["x"].t.dtype, inp["x"].t.device, fill=cr.QNAN)
    x.t[:live] = inp["x"].t[:live]
    return dict(inp, x=x)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_static_launch_of_every_tile(name, fp16):
    """rows_dyn = NULL: for mask.deconv the static pixel shuffle; for mask.conv the launches the counted ones are compared with."""
    L, inp, ref, accepted, fails, ys = _static(name, fp16)
    assert not fails, "\n".join(fails)
    assert accepted == [c for c in cr.SWEEP_IDS if cr.tile_runs(c, L, fp16, B, dyn=False)]
    assert set(cr.tuner_ids(L, fp16, B, dyn=False)) <= set(accepted)
    assert all(y.pattern_count() == 0 for y in ys.values())


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_device_row_count_on_every_tile(name, fp16, count):
    L, inp, ref, st_accepted, st_fails, st_ys = _static(name, fp16)
    assert not st_fails, "\n".join(st_fails)
    live = min(count, B)
    dead = _with_dead_rois(L, inp, live)
    count_t = torch.tensor([count], dtype=torch.int32, device="cuda")
    print(f"\n[{name} {'fp16' if fp16 else 'fp32'} count {count}] live rows {live * L.Ho * L.Wo} of {B * L.Ho * L.Wo}")
    accepted, fails, ys = _run_ids(L, dead, ref, count_t, live * L.Ho * L.Wo, f"count {count}")
    assert int(count_t.item()) == count and dead["x"].guards_intact()
    assert accepted == [c for c in cr.SWEEP_IDS if cr.tile_runs(c, L, fp16, B, dyn=True)]
    assert set(cr.tuner_ids(L, fp16, B, dyn=True)) <= set(accepted)
    assert set(accepted) <= set(st_accepted)
    for cfg, y in ys.items():
        if live == 0 and y.pattern_count() != y.n:
            fails.append(f"tile {cfg}: {y.n - y.pattern_count()} elements written at count 0")
        if not torch.equal(_bits(y, live), _bits(st_ys[cfg], live)):       # the first `live` images of y as stored, either layout
            fails.append(f"tile {cfg}: {int((_bits(y, live) != _bits(st_ys[cfg], live)).sum())} live elements differ from the static launch")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_filter_stationary_tile_refuses_a_device_row_count(fp16):
    """Tile 33 sizes its grid and its store loop from the host row count: conv_bs_ok refuses m_dyn by name (neither mask-head
    shape can run it at all, so this plain 1x1 layer is what reaches that rule)."""
    L = cr.Conv("one", 128, 256, 1, 1, 0, 14, 14, scale=False)
    assert cr.tile_runs(33, L, fp16, B) and not cr.tile_runs(33, L, fp16, B, dyn=True)
    inp = cr.make_inputs(L, fp16, B, "cuda", seed=5)
    ref = cr.reference(L, inp, torch.arange(B * L.Ho * L.Wo))
    y = cr.new_output(L, inp)
    cr.launch(L, inp, y, 33, strict=True, rows_entry=True)
    v = cr.check(L, y, ref)
    assert v.ok, v.why
    y = cr.new_output(L, inp)
    with pytest.raises(Exception, match="tile_cfg 33 cannot run"):
        cr.launch(L, inp, y, 33, strict=True, count=torch.tensor([3], dtype=torch.int32, device="cuda"))
    assert y.guards_intact() and y.pattern_count() == y.n


def test_print_the_measured_table():
    """(runs last in this file) the worst err/bound and RMS per layer and output dtype over every id and count, for the record."""
    for (name, dt), (eb, rms) in sorted(WORST.items()):
        print(f"\n[table] {name:12s} {dt:8s} worst err/bound {eb:.3g}  worst RMS {rms:.3g}")
    assert all(eb <= 1.0 for eb, _ in WORST.values())
