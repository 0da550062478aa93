"""The 36 plane contractions of the unfolded F(4x4,3x3) form on the split-bf16 tiles (conv_split.hip's batched launch; op-level
entry td_conv2d_winograd_nhwc / _head_nhwc under TD_WINO_TILE=4 TD_WINO_FOLD=0 TD_WINO_SPLIT=1): finite everywhere on a NaN-filled
output, deterministic, tile ids 34 - 37 bit-equal to each other, within the project's F(4x4) tolerance 5e-5 * max(1, max|ref|) of
float64 (printed beside the fp32-plane form's error on the same inputs) and NOT bit-equal to the fp32-plane form; a batch of 2
equals its two images run alone; the head in the output transform equals the split three-launch form followed by the 1x1 head."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Cin, H, W, Cout, scale, bias, relu)
CASES = [
    (1, 256, 13, 13, 256, False, False, False),       # T = 16: every row tile partial
    (2, 256, 25, 25, 256, False, True, True),         # T = 98: one full and one partial 64-row tile
    (1, 512, 25, 25, 512, True, True, True),          # K = 512, res5's planes
    (1, 128, 47, 61, 160, False, False, False),       # 4 k-chunks (the loop's it+1 / it+2 tails), Cout no multiple of a block width, border tiles
    (3, 256, 50, 50, 256, False, False, False),       # T = 507: several row tiles
]
IDS = ["T16", "T98.bias.relu", "K512.scale.bias.relu", "C128.N160.border", "T507"]
SPLIT_ENV = {"TD_WINO_TILE": "4", "TD_WINO_FOLD": "0", "TD_WINO_SPLIT": "1"}
FP32_ENV = {"TD_WINO_TILE": "4", "TD_WINO_FOLD": "0"}

_INPUTS = {}


def _inputs(i):
    """x mostly positive (as post-ReLU maps are), w / sqrt(9 C): the inputs of test_winograd_f4x4_conv_matches_torch; the float64
    reference is computed once per case and never written to."""
    if i not in _INPUTS:
        B, Cin, H, W, Cout, use_scale, use_bias, relu = CASES[i]
        rng = np.random.default_rng(4300 + i)
        x = np.maximum(rng.standard_normal((B, Cin, H, W), dtype=np.float32), -0.5)
        w = rng.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.float32(np.sqrt(Cin * 9))
        scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32) if use_scale else None
        bias = rng.standard_normal(Cout).astype(np.float32) if use_bias else None
        ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None, stride=1, padding=1)
        if use_scale:
            ref = ref * torch.from_numpy(scale).double().reshape(1, -1, 1, 1)
        if use_bias:
            ref = ref + torch.from_numpy(bias).double().reshape(1, -1, 1, 1)
        if relu:
            ref = F.relu(ref)
        ref = ref.numpy()
        ref.setflags(write=False)
        _INPUTS[i] = (x, w, scale, bias, ref)
    return _INPUTS[i]


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)


def _wino(x, w, scale, bias, relu, env):
    """x [B,C,H,W], w [N,C,3,3] numpy → y [B,H,W,N] torch (cuda) through td_conv2d_winograd_nhwc on a NaN-filled output"""
    from treedetection_amd import _lib
    from tests.gpu_util import dev
    lib = _lib.load()
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xd, wd = dev(x.transpose(0, 2, 3, 1)), dev(w.transpose(0, 2, 3, 1))
    sd = dev(scale) if scale is not None else None
    bd = dev(bias) if bias is not None else None
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    y = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device="cuda")
    with _Env(env):
        _lib.check(lib.td_conv2d_winograd_nhwc(p(xd), p(wd), p(sd), p(bd), y.data_ptr(), B, H, W, Cin, Cout, int(relu), _lib.stream_ptr()),
                   "td_conv2d_winograd_nhwc")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_split_planes(i):
    relu = CASES[i][7]
    x, w, scale, bias, ref = _inputs(i)
    y = _wino(x, w, scale, bias, relu, SPLIT_ENV)
    assert torch.isfinite(y).all(), "the split-plane output is not finite everywhere"
    assert torch.equal(y, _wino(x, w, scale, bias, relu, SPLIT_ENV)), "two runs differ"
    for cfg in ("34", "35", "36", "37"):
        yc = _wino(x, w, scale, bias, relu, dict(SPLIT_ENV, TD_CONV_CFG=cfg))
        assert torch.equal(y, yc), f"tile id {cfg} differs from the default split tile"
    y32 = _wino(x, w, scale, bias, relu, FP32_ENV)
    tol = 5e-5 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(y.cpu().numpy().transpose(0, 3, 1, 2) - ref).max())
    err32 = float(np.abs(y32.cpu().numpy().transpose(0, 3, 1, 2) - ref).max())
    print(f"\n[{IDS[i]}] max |err| against float64: split planes {err:.3g}, fp32 planes {err32:.3g} (tolerance {tol:.3g})")
    assert err <= tol, f"max abs err {err} > {tol}"
    assert not torch.equal(y, y32), "bit-equal to the fp32-plane form: the split planes did not run"


def test_batch_of_two_equals_its_images_alone():
    x, w, scale, bias, _ = _inputs(1)
    y = _wino(x, w, scale, bias, True, SPLIT_ENV)
    for b in range(2):
        yb = _wino(x[b:b + 1], w, scale, bias, True, SPLIT_ENV)
        assert torch.equal(y[b:b + 1], yb), f"image {b} of the batch differs from the image run alone"


@pytest.mark.parametrize("case", [(2, 256, 25, 25, 15), (1, 256, 13, 19, 15)], ids=["25x25", "13x19"])
def test_head_in_transform_equals_split_form_then_head(case):
    """The head rides in the output transform, which reads M as before: bit-identical to the split three-launch form written out
    followed by the 1x1 head as a conv_igemm launch (tests/test_conv_gpu.py states the same for the fp32 planes)."""
    from treedetection_amd import _lib
    from tests.gpu_util import conv2d_hip, dev
    B, Cin, H, W, n = case
    rng = np.random.default_rng(977 + H)
    x = np.maximum(rng.standard_normal((B, Cin, H, W), dtype=np.float32), -0.5)
    w = rng.standard_normal((256, Cin, 3, 3), dtype=np.float32) / np.float32(np.sqrt(Cin * 9))
    bias = rng.standard_normal(256).astype(np.float32)
    hw = rng.standard_normal((n, 256, 1, 1), dtype=np.float32) / np.float32(16.0)
    hb = rng.standard_normal(n).astype(np.float32)
    lib = _lib.load()
    y = _wino(x, w, None, bias, True, SPLIT_ENV)
    assert not torch.equal(y, _wino(x, w, None, bias, True, FP32_ENV))
    ref = conv2d_hip(y.cpu().numpy().transpose(0, 3, 1, 2), hw, bias=hb, precision=0, tile_cfg=3)
    xd, wd, bd = dev(x.transpose(0, 2, 3, 1)), dev(w.transpose(0, 2, 3, 1)), dev(bias)
    hwd, hbd = dev(hw.reshape(n, 256)), dev(hb)
    got = torch.full((B, H, W, n), float("nan"), dtype=torch.float32, device="cuda")
    with _Env(SPLIT_ENV):
        _lib.check(lib.td_conv2d_winograd_head_nhwc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), hwd.data_ptr(), hbd.data_ptr(), got.data_ptr(),
                                                    B, H, W, Cin, n, _lib.stream_ptr()), "td_conv2d_winograd_head_nhwc")
    torch.cuda.synchronize()
    g = got.cpu().numpy().transpose(0, 3, 1, 2)
    assert not np.isnan(g).any() and np.array_equal(g, ref), float(np.abs(g - ref).max())
    assert np.abs(ref).max() > 0.5
