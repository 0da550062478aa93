"""The 128 x 256 split-bf16 tile with tall waves (conv_split.hip, tile id 34: conv_split_kernel<4, 2, 1, 4, 1>, 1 x 4 waves of
128 x 64) through td_conv2d_nhwc against the float64 reference of tests/conv_ref.py — its bound and RMS_MAX unchanged — and bit
equality with tiles 35 and 37 on the same inputs.

tests/test_conv_split_gpu.py runs id 34 on the shared cases; these are the shapes only this geometry can get wrong (every wave
holds all 128 rows of the block as four 32-row tiles and 64 of its 256 columns as two 32-column tiles):
  t130x72        M 130, K 32, N 72: one k-chunk (the prologue and one trip with both nested ifs skipped), a second row block with two
                 live rows, wave 1 with eight live columns, waves 2 and 3 with none;
  t100x256.res   M 100, K 64, N 256, shortcut and ReLU: rows that exist only in the wave's third and fourth row tiles (64 - 95, 96 -
                 99), two k-chunks (one nested `if` of the unrolled loop taken), every wave with live columns;
  t128x264.s2    M 128 exactly (two 15 x 15 maps at stride 2 -> 8 x 8), K 128, N 264: four k-chunks (a second loop trip of one chunk), a
                 second column block of eight columns, the strided row addressing;
  s256x64.up2    the top-down-add form (nearest-2x shortcut) of tests/conv_split_cases.py at M 288: three row blocks, the last partial;
  device rows    td_conv2d_rows_nhwc with a device row count that cuts the block at row 65 (one row of the third row tile) and one
                 of 0: the rows at and past the count hold NaN in x and must keep the sentinel in y."""
import pytest
import torch

from tests import conv_ref as cr
from tests.conv_split_cases import SHORT_K

pytestmark = pytest.mark.gpu

TILE, TWINS = 34, (35, 37)    # 128x256 of 128 x 64 waves; 128x128 and 64x128 of 64 x 64 waves

CASES = [
    (cr.Conv("t130x72", 32, 72, 1, 1, 0, 5, 13), 2),
    (cr.Conv("t100x256.res", 64, 256, 1, 1, 0, 10, 10, res=1), 1),
    (cr.Conv("t128x264.s2", 128, 264, 1, 2, 0, 15, 15), 2),
    SHORT_K[3],
]
assert [B * L.Ho * L.Wo for L, B in CASES] == [130, 100, 128, 288] and CASES[3][0].res == 2
ROWS_LAYER, ROWS_B = cr.Conv("t130x96.rows", 96, 96, 1, 1, 0, 5, 13), 2      # M 130, three k-chunks (one full trip of the unrolled loop)
ROW_COUNTS = [65, 0]


def _bits(g):
    return g.t.reshape(-1).view(g.ity)


@pytest.mark.parametrize("L,B", CASES, ids=[L.name for L, _ in CASES])
def test_tile34_against_float64_and_tiles_35_37(L, B):
    seed = 211 + L.Cin
    inp = cr.make_inputs(L, False, B, "cuda", seed)
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed))
    out = {}
    print(f"\n[{L.name} B={B}] M={B * L.Ho * L.Wo} K={L.K} N={L.Cout}")
    for cfg in (TILE,) + TWINS:
        y = cr.new_output(L, inp)
        cr.launch(L, inp, y, cfg, strict=True)
        v = cr.check(L, y, ref)
        print(f"  tile {cfg}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        assert v.ok, f"tile {cfg}: {v.why}"
        out[cfg] = y
    for twin in TWINS:
        assert torch.equal(_bits(out[TILE]), _bits(out[twin])), f"tile {TILE} differs from tile {twin}"


@pytest.mark.parametrize("count", ROW_COUNTS)
def test_tile34_with_a_device_row_count(count):
    L, B = ROWS_LAYER, ROWS_B
    M = B * L.Ho * L.Wo
    inp = cr.make_inputs(L, False, B, "cuda", 977)
    ref = cr.reference(L, inp, torch.arange(M))
    dead = cr.Guarded(tuple(inp["x"].t.shape), torch.float32, "cuda", fill=cr.QNAN)      # rows at and past the count: quiet NaN
    dead.t.reshape(M, L.Cin)[:count] = inp["x"].t.reshape(M, L.Cin)[:count]
    inp = dict(inp, x=dead)
    count_t = torch.tensor([count], dtype=torch.int32, device="cuda")
    out = {}
    print(f"\n[{L.name} count {count}] live rows {count} of {M}")
    for cfg in (TILE,) + TWINS:
        y = cr.new_output(L, inp)
        cr.launch(L, inp, y, cfg, strict=True, count=count_t, rows_mul=1)
        v = cr.check(L, y, ref, live_rows=count)
        print(f"  tile {cfg}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        assert v.ok, f"tile {cfg}: {v.why}"
        assert y.pattern_count() == (M - count) * L.Cout, f"tile {cfg}: rows at or past the count were written, or live ones were not"
        out[cfg] = y
    assert int(count_t.item()) == count and dead.guards_intact()
    for twin in TWINS:
        assert torch.equal(_bits(out[TILE]), _bits(out[twin])), f"tile {TILE} differs from tile {twin}"
