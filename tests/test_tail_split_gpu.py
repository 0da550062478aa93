"""The split form of the fp32 bottleneck tail (bottleneck.hip: the 3x3 of conv2 on the bf16 matrix cores with three-piece operands,
the 1x1 of conv3 as in the fp32 tail) through td_bottleneck_tail_split_nhwc, mid = 64, cout = 256, in both of its modes.

Blocks are 64 rows of the flat pixel index, four waves: wave (wm, wk) contracts rows 32 wm .. + 31 with channel chunk wk of every
tap, and the two chunk sums meet through LDS. Shapes for where that can go wrong:
  B 1,  8 x  8  (M  64)  one block, every pixel on a border, every padding tap;
  B 2,  7 x  9  (M 126)  a block holds rows of two images (no tap may reach into the neighbouring image), the last block partial;
  B 1, 13 x 10  (M 130)  full blocks plus a two-row tail;
  B 2, 16 x 24  (M 768)  interior pixels, twelve blocks, the XCD remap.
(The block is 64 rows, so the issue's extra cases for other block sizes do not apply.)

Per case, with the sentinel / guard buffers of tests/conv_ref.py (x and the shortcut wrapped in quiet NaN):
  (a) the mid tensor of the mid-store mode against the float64 3x3 + scale + bias + ReLU of EVERY row: cr.check's bound and RMS
      criterion, RMS_MAX unchanged, K = 576;
  (b) the fused output bit-equal to the mid-store launch followed by td_conv2d_nhwc (1x1, scale, bias, shortcut, ReLU; fp32 tile 0);
  (c) guards intact around mid and y (nothing at or past M written), no sentinel left, nothing non-finite;
  (d) the fused output NOT bit-equal to td_bottleneck_tail_nhwc (fp32) on the same inputs, and both inside one float64 bound of
      the two layers chained. That bound is tests/conv_ref.py's, applied twice: with mid64 / b2 the float64 mid tensor and its
      per-element bound from (a), S = (|mid64| + b2) |W3|^T, gamma = 1.05 * 64 * 2^-24, A = |s3| S (1 + gamma) + |b3| + |shortcut|,
          |y - y64| <= |s3| (b2 |W3|^T)  +  gamma |s3| S  +  4 * 2^-24 A
      — the mid tensor's error carried through the 1x1 (ReLU is 1-Lipschitz), the 64-term fp32 dot product in any order, and the
      epilogue's roundings."""
import pytest
import torch

from tests import conv_ref as cr

pytestmark = pytest.mark.gpu

MID, COUT = 64, 256
CASES = [(1, 8, 8), (2, 7, 9), (1, 13, 10), (2, 16, 24)]
assert [b * h * w for b, h, w in CASES] == [64, 126, 130, 768]


def _bits(g):
    return g.t.reshape(-1).view(g.ity)


def _p(t):
    return t.data_ptr() if t is not None else None


def _split_tail(inp2, inp3, B, H, W, y=None, mid=None):
    from treedetection_amd import _lib
    lib = _lib.load()
    if mid is not None:
        st = lib.td_bottleneck_tail_split_nhwc(_p(inp2["x"]), _p(inp2["w"]), _p(inp2["scale"]), _p(inp2["bias"]), None, None, None, None, None,
                                               _p(mid), B, H, W, MID, COUT, _lib.stream_ptr())
    else:
        st = lib.td_bottleneck_tail_split_nhwc(_p(inp2["x"]), _p(inp2["w"]), _p(inp2["scale"]), _p(inp2["bias"]), _p(inp3["w"]),
                                               _p(inp3["scale"]), _p(inp3["bias"]), _p(inp3["res"]), _p(y), None, B, H, W, MID, COUT,
                                               _lib.stream_ptr())
    _lib.check(st, "td_bottleneck_tail_split_nhwc")
    torch.cuda.synchronize()


def _clean(g, what):
    assert g.guards_intact(), f"{what}: a guard zone (rows at or past M) was written"
    assert g.pattern_count() == 0, f"{what}: {g.pattern_count()} elements never written"
    assert bool(torch.isfinite(g.t).all().item()), f"{what}: non-finite values"


@pytest.mark.parametrize("B,H,W", CASES, ids=[f"B{b}.{h}x{w}" for b, h, w in CASES])
def test_split_tail_mid_store_fused_twin_and_bound(B, H, W):
    from treedetection_amd import _lib
    M = B * H * W
    L2 = cr.Conv("tail.conv2", MID, MID, 3, 1, 1, H, W)
    L3 = cr.Conv("tail.conv3", MID, COUT, 1, 1, 0, H, W, res=1)
    seed = 1000 * B + 10 * H + W
    inp2 = cr.make_inputs(L2, False, B, "cuda", seed)
    inp3 = cr.make_inputs(L3, False, B, "cuda", seed + 1)
    rows = torch.arange(M)
    ref2 = cr.reference(L2, inp2, rows)

    # (a), (c): the mid-store mode
    mid = cr.new_output(L2, inp2)
    _split_tail(inp2, inp3, B, H, W, mid=mid)
    v = cr.check(L2, mid, ref2)
    print(f"\n[B={B} {H}x{W}] M={M}  mid: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
    assert v.ok, v.why

    # (b), (c): fused == mid-store launch, then the fp32 1x1 with shortcut
    inp3m = dict(inp3, x=mid)
    two = cr.new_output(L3, inp3m)
    cr.launch(L3, inp3m, two, 0, strict=True)
    torch.cuda.synchronize()
    y = cr.new_output(L3, inp3m)
    _split_tail(inp2, inp3, B, H, W, y=y)
    for g, what in ((mid, "mid"), (two, "two launches"), (y, "fused")):
        _clean(g, what)
    assert inp2["x"].guards_intact() and inp3["res"].guards_intact()
    assert torch.equal(_bits(y), _bits(two)), f"fused differs from mid-store + 1x1 in {int((_bits(y) != _bits(two)).sum())} elements"

    # (d): not the fp32 tail's bits, and both inside the chained float64 bound
    lib = _lib.load()
    y32 = cr.new_output(L3, inp3m)
    _lib.check(lib.td_bottleneck_tail_nhwc(_p(inp2["x"]), _p(inp2["w"]), _p(inp2["scale"]), _p(inp2["bias"]), _p(inp3["w"]), _p(inp3["scale"]),
                                           _p(inp3["bias"]), _p(inp3["res"]), _p(y32), B, H, W, MID, COUT, 0, _lib.stream_ptr()),
               "td_bottleneck_tail_nhwc")
    torch.cuda.synchronize()
    _clean(y32, "fp32 tail")
    assert not torch.equal(_bits(y), _bits(y32)), "the split tail equals the fp32 tail bit for bit: the split 3x3 did not run"
    W3 = inp3["w"].reshape(COUT, MID).cpu().double()
    s3, b3 = inp3["scale"].cpu().double(), inp3["bias"].cpu().double()
    rr = inp3["res"].t.reshape(M, COUT).cpu().double()
    mid64, bnd2 = ref2.y64, ref2.bound
    y64 = (mid64 @ W3.T * s3 + b3 + rr).clamp_min(0)
    S = (mid64.abs() + bnd2) @ W3.abs().T
    gamma = 1.05 * MID * cr.U32
    A = s3.abs() * S * (1 + gamma) + b3.abs() + rr.abs()
    bound = s3.abs() * (bnd2 @ W3.abs().T) + gamma * s3.abs() * S + 4 * cr.U32 * A
    for g, what in ((y, "split tail"), (y32, "fp32 tail")):
        ratio = ((g.t.reshape(M, COUT).cpu().double() - y64).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"  {what}: err/bound {ratio:.3g}")
        assert ratio <= 1.0, f"{what}: outside the chained float64 bound ({ratio:.3g})"
