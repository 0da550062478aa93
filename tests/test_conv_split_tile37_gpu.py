"""The 64 x 128 split-bf16 tile (conv_split.hip, tile id 37: conv_split_kernel<2, 2, 1, 2, 2>, two waves of 64 x 64) through
td_conv2d_nhwc against the float64 reference of tests/conv_ref.py — its bound and RMS_MAX unchanged —, bit equality with tile 35
on the same inputs, and the refusals.

Shapes: the four short-K ones of tests/conv_split_cases.py and two more. Together: k-chunk counts (32 floats) 2, 1, 4, 8, 3 and 12,
so every remainder by the three LDS stages of the k loop; M below one 64-row block (15 rows); ragged M (494, 338, 126 rows: 8, 6
and 2 row blocks, the last partial); partial 32-column tiles (40, 48 channels: the wave's second tile is past Cout or half empty);
two 128-column blocks with the last one partial (160 = 128 + 32); stride 2; both shortcut modes (same size, nearest 2x)."""
import pytest
import torch

from tests import conv_ref as cr
from tests.conv_split_cases import NS, SHORT_K

pytestmark = pytest.mark.gpu

TILE, TWIN = 37, 35           # 64x128 and 128x128: the same 64 x 64 wave tile, one and two wave rows

CASES = SHORT_K + [
    (cr.Conv("s96x40", 96, 40, 1, 1, 0, 9, 11), 1),
    (cr.Conv("s384x160.res", 384, 160, 1, 1, 0, 7, 9, res=1), 2),
]
_CHUNKS = {L.Cin // 32 for L, _ in CASES}
assert _CHUNKS == {1, 2, 3, 4, 8, 12} and {c % NS for c in _CHUNKS} == set(range(NS))


@pytest.mark.parametrize("L,B", CASES, ids=[L.name for L, _ in CASES])
def test_tile37_against_float64_and_tile35(L, B):
    seed = 101 + L.Cin
    inp = cr.make_inputs(L, False, B, "cuda", seed)
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed))
    out = {}
    print(f"\n[{L.name} B={B}] M={B * L.Ho * L.Wo} K={L.K} N={L.Cout}")
    for cfg in (TILE, TWIN):
        y = cr.new_output(L, inp)
        cr.launch(L, inp, y, cfg, strict=True)
        v = cr.check(L, y, ref)
        print(f"  tile {cfg}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        assert v.ok, f"tile {cfg}: {v.why}"
        out[cfg] = y
    assert torch.equal(out[TILE].t.view(out[TILE].ity), out[TWIN].t.view(out[TWIN].ity)), f"tile {TILE} differs from tile {TWIN}"


def test_tile37_is_refused_on_3x3_and_fp16():
    for L, fp16 in ((cr.Conv("r3x3", 64, 64, 3, 1, 1, 8, 8), False), (cr.Conv("r16", 64, 64, 1, 1, 0, 8, 8), True)):
        inp = cr.make_inputs(L, fp16, 1, "cuda", 3)
        with pytest.raises(Exception, match=f"tile_cfg {TILE} cannot run"):
            cr.launch(L, inp, cr.new_output(L, inp), TILE, strict=True)
