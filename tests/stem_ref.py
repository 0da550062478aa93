"""A float64 checker for the input side of the network (treedetection_amd/csrc/stem.hip): stem_conv_kernel in its four
forms, stem_mfma_kernel, maxpool3x3s2_kernel and subsample2_kernel (plain module, imported by tests/test_stem_gpu.py; the
CPU half runs in the mutation controls of tests/test_stem_ref.py). Everything is float64 on the CPU (torch conv2d).

The true operation. detectron2 normalises, then pads: x = pixel - mean inside [0, vh) x [0, vw) of each image and 0
everywhere else — the 3-pixel frame of the convolution and the area between the valid and the padded size alike. mean is
the kernel's float32 constants (103.530f, 116.280f, 123.675f, BGR order); scale and bias are folded from the state dict in
the float32 steps of engine.cpp's bn_fold (r = 1 / sqrt(var + 1e-5f), s = g r, bias = b - m s) and then taken as exact.

    y64 = relu(scale conv(x, W) + bias),   S = conv(|x|, |W|)                       (7x7, stride 2, pad 3)

Bound of stem_conv_kernel, every form (the form of tests/conv_ref.py): u = 2^-24, gamma = 1.05 (147 + 2) u — 147 terms in
any summation order, one more for the rounding of x - mean, one for a one-ulp difference in scale —,
A = |scale| S (1 + gamma) + |bias|:

    |y - y64| <= gamma |scale| S + 4 u A   [ + 2^-11 (|y64| + gamma |scale| S + 4 u A) + 2^-25  for fp16 outputs ]

stem_mfma_kernel has two references.
  * Model, the kernel's own stated arithmetic: raw pixels (0..255) x fp16-rounded filters w16, fp16(mean) = (103.5, 116.25,
    123.6875) at every tap outside the valid rectangle, bias' = float32(bias - scale sum w16 mean) computed as
    stem_mfma_prepare does (float64, means 103.530 / 116.280 / 123.675, rounded once). S_m = conv(|taps|, |w16|); the bound
    has the same form with gamma = 1.05 (256 + 2) u (the padded k axis) and always the fp16 output term. |bias'| carries the
    folded mean, so 4 u A covers the cancellation of scale conv(taps) against it.
  * Truth: y64 above with the unrounded filters. Allowed distance = the model bound
    + |scale| (conv(|x|, |w16 - W|) + conv(outside |fp16(mean) - mean|, |w16|)): the filter rounding and the padding value,
    both exact per output (ReLU is 1-Lipschitz, so they carry through it).

Sentinels. uint8 batches hold seeded random bytes outside each image's valid rectangle, float batches NaN: a tap read
there moves (or poisons) an output, and the comparison `err <= bound` is false for NaN.

Teeth. In every case at least MIN_POSITIVE of the reference outputs inside the valid area are positive (else ReLU hides
errors); asserted on the reference alone. Uniform random bytes with make_synthetic_state_dict(50, seed=3, width_div=2) or
(50, seed=5) give about 50 % (0.49-0.55 over the cases here).

Measured worst err / bound (for information: nothing is fitted to them, the bounds are derived).
  CPU (tests/test_stem_ref.py, B = 3, 64 x 96, both seeded networks): float32 emulation of the true operation 0.020-0.023
  (0.92-0.95 once rounded to fp16: half an fp16 ulp is the whole of that bound); float32-accumulate emulation of the model,
  rounded to fp16, 0.81-0.82 of the model bound; the model against the truth 0.55 of the extra term alone. Mutants: padding
  normalised 3e8-5e9, valid sizes ignored 2e9-1e10, valid height off by one 4e8-2e9 (on the edge rows only), RGB mean
  3e4-4e4, fp16(mean) for every pixel 73-101, filter row ky = 6 dropped 6e4.
  MI355X (tests/test_stem_gpu.py, worst over the geometries and the input formats each engine takes): GPU_MEASURED below.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U16 = 2.0 ** -11
K_VALU = 147
K_MFMA = 256
MIN_POSITIVE = 0.30
MEAN32 = np.array([103.530, 116.280, 123.675], dtype=np.float32)          # the kernels' constants, BGR
MEAN16 = MEAN32.astype(np.float16)                                        # 103.5, 116.25, 123.6875
MEAN_PREPARE = np.array([103.530, 116.280, 123.675], dtype=np.float64)    # stem_mfma_prepare's doubles
INPUT_F32_CHW, INPUT_U8_HWC = 0, 1

# worst err / bound per engine on an MI355X, over every geometry (and both input formats where the engine takes both)
GPU_MEASURED = {
    "fp32, 32 channels": 0.087, "fp32, 64 channels": 0.054,                    # stem_conv_kernel, fp32 outputs
    "fp16, 32 channels": 0.958, "fp16, 64 channels, VALU": 0.966,              # … fp16 outputs: the output rounding dominates
    "fp16, 64 channels, MFMA engine, float input": 0.91,                       # (stem_conv_kernel again)
    "fp16 MFMA against the model": 0.839, "fp16 MFMA against the truth": 0.64,
}

# the geometries of the GPU tests: (B, Hp, Wp, valid sizes)
SEAM = (13, 16, 19, 29, 32, 35, 61, 64, 67)
GEOMETRIES = {
    "mixed": (3, 64, 96, ((64, 96), (37, 50), (1, 1))),
    # valid edges on, just before and just after the 32-pixel seam of the 16 x 16 VALU tile and the 16 x 32 seam of the MFMA tile
    "seams": (4, 96, 160, ((13, 67), (32, 35), (61, 16), (64, 29))),
    "seams2": (4, 96, 160, ((16, 64), (19, 61), (29, 19), (67, 13))),
    "seams3": (4, 96, 160, ((35, 32), (67, 67), (64, 16), (16, 64))),
    # 7 x 16 x 8 = 896 MFMA tiles against 768 resident blocks: some blocks walk a second tile through the prefetch
    "walk": (7, 256, 256, ((256, 256), (201, 131), (32, 256), (256, 35), (1, 1), (255, 255), (129, 250))),
}


@dataclasses.dataclass(frozen=True)
class Params:
    W: torch.Tensor          # [C, 3, 7, 7] float64 (the float32 filters, exact)
    scale: torch.Tensor      # [C] float64 (the float32 fold, exact)
    bias: torch.Tensor
    w16: torch.Tensor        # the filters rounded to fp16
    bias16: torch.Tensor     # stem_mfma_prepare's bias'


def stem_params(sd) -> Params:
    p = "backbone.bottom_up.stem.conv1"
    w = np.ascontiguousarray(sd[p + ".weight"], dtype=np.float32)
    g, b, m, v = (np.ascontiguousarray(sd[f"{p}.norm.{k}"], dtype=np.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    r = np.float32(1.0) / np.sqrt(v + np.float32(1e-5))
    s = g * r
    bias = b - m * s
    assert r.dtype == s.dtype == bias.dtype == np.float32
    w16 = w.astype(np.float16).astype(np.float64)
    corr = (w16 * MEAN_PREPARE[None, :, None, None]).sum(axis=(1, 2, 3))
    bias16 = (bias.astype(np.float64) - s.astype(np.float64) * corr).astype(np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))      # noqa: E731
    return Params(t(w), t(s), t(bias), t(w16), t(bias16))


def make_batch(fmt: int, B: int, Hp: int, Wp: int, valid, seed: int) -> np.ndarray:
    """uint8 [B, Hp, Wp, 3] of seeded random bytes (the bytes outside the valid rectangles are the sentinels), or float32
    [B, 3, Hp, Wp] of non-integers in [0, 255] with NaN outside the valid rectangles."""
    assert len(valid) == B and Hp % 32 == 0 and Wp % 32 == 0 and Hp >= 64 and Wp >= 64
    rng = np.random.default_rng(seed)
    if fmt == INPUT_U8_HWC:
        return rng.integers(0, 256, (B, Hp, Wp, 3), dtype=np.uint8)
    x = (rng.integers(0, 255, (B, 3, Hp, Wp)) + rng.uniform(0.05, 0.95, (B, 3, Hp, Wp))).astype(np.float32)
    assert (x != np.rint(x)).all() and x.min() >= 0 and x.max() <= 255
    for b, (vh, vw) in enumerate(valid):
        x[b, :, vh:, :] = np.nan
        x[b, :, :, vw:] = np.nan
    return x


def pixels(batch: np.ndarray, valid):
    """→ (float64 [B, 3, Hp, Wp] pixel values with 0 outside the valid rectangles, inside mask [B, 1, Hp, Wp])."""
    p = torch.from_numpy(batch.transpose(0, 3, 1, 2).astype(np.float64) if batch.dtype == np.uint8 else batch.astype(np.float64))
    B, _, Hp, Wp = p.shape
    mask = torch.zeros((B, 1, Hp, Wp), dtype=torch.float64)
    for b, (vh, vw) in enumerate(valid):
        mask[b, :, :vh, :vw] = 1.0
    return torch.where(mask > 0, p, torch.zeros((), dtype=torch.float64)), mask


def _conv(x, w):
    return F.conv2d(x, w, stride=2, padding=3)


def _chan(v):
    return v[None, :, None, None]


def _with_out_rounding(y, bound):
    return bound + U16 * (y.abs() + bound) + 2.0 ** -25


@dataclasses.dataclass
class Reference:
    y64: torch.Tensor        # [B, C, Ho, Wo] float64
    bound: torch.Tensor      # per-element bound for fp32 outputs
    bound16: torch.Tensor    # … for fp16 outputs
    positive: float          # share of positive outputs inside the valid area


def valid_outputs(mask):
    """[B, 1, Ho, Wo] bool: outputs whose centre tap (2 oy, 2 ox) lies inside the valid rectangle."""
    return mask[:, :, ::2, ::2] > 0


def reference(P: Params, pix, mask) -> Reference:
    """The true operation and the bound of stem_conv_kernel (see the module docstring)."""
    x = (pix - _chan(torch.from_numpy(MEAN32.astype(np.float64)))) * mask
    sc, bi = _chan(P.scale), _chan(P.bias)
    y = (sc * _conv(x, P.W) + bi).clamp_min(0)
    S = _conv(x.abs(), P.W.abs())
    gamma = 1.05 * (K_VALU + 2) * U32
    A = sc.abs() * S * (1 + gamma) + bi.abs()
    bound = gamma * sc.abs() * S + 4 * U32 * A
    inside = valid_outputs(mask).expand_as(y)
    return Reference(y, bound, _with_out_rounding(y, bound), float((y[inside] > 0).double().mean()))


def mfma_taps(pix, mask):
    """[B, 3, Hp + 6, Wp + 6]: raw pixels inside the valid rectangles, fp16(mean) at every other tap, frame included."""
    m16 = _chan(torch.from_numpy(MEAN16.astype(np.float64)))
    B, _, Hp, Wp = pix.shape
    taps = m16.expand(B, 3, Hp + 6, Wp + 6).clone()
    taps[:, :, 3:Hp + 3, 3:Wp + 3] = pix * mask + m16 * (1 - mask)
    return taps


@dataclasses.dataclass
class MfmaReference:
    model: torch.Tensor          # the kernel's stated arithmetic in float64
    model_bound: torch.Tensor    # |kernel - model| <=
    extra: torch.Tensor          # filter rounding + padding value: |model - truth| <= extra (+ roundings inside model_bound)
    truth_bound: torch.Tensor    # |kernel - truth| <= model_bound + extra


def mfma_reference(P: Params, pix, mask) -> MfmaReference:
    assert bool((pix == pix.round()).all()), "the MFMA stem takes uint8 pixels"
    sc, bi = _chan(P.scale), _chan(P.bias16)
    taps = mfma_taps(pix, mask)
    y = (sc * F.conv2d(taps, P.w16, stride=2) + bi).clamp_min(0)
    S = F.conv2d(taps.abs(), P.w16.abs(), stride=2)
    gamma = 1.05 * (K_MFMA + 2) * U32
    A = sc.abs() * S * (1 + gamma) + bi.abs()
    model_bound = _with_out_rounding(y, gamma * sc.abs() * S + 4 * U32 * A)
    x = (pix - _chan(torch.from_numpy(MEAN32.astype(np.float64)))) * mask
    B, _, Hp, Wp = pix.shape
    outside = torch.ones((B, 1, Hp + 6, Wp + 6), dtype=torch.float64)
    outside[:, :, 3:Hp + 3, 3:Wp + 3] = 1 - mask
    dmean = _chan(torch.from_numpy(np.abs(MEAN16.astype(np.float64) - MEAN32.astype(np.float64))))
    extra = sc.abs() * (_conv(x.abs(), (P.w16 - P.W).abs()) + F.conv2d(outside * dmean, P.w16.abs(), stride=2))
    return MfmaReference(y, model_bound, extra, model_bound + extra)


def worst_ratio(got, want, bound):
    """got [B, C, Ho, Wo] (any float dtype) against a reference: → (every element inside, worst err / bound, where).
    A NaN in `got` is outside whatever the bound."""
    err = (got.double() - want).abs()
    ok = err <= bound
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300))
    i = int(ratio.argmax())
    where = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    return bool(ok.all()), float(ratio.reshape(-1)[i]), where


def nchw(t: torch.Tensor) -> torch.Tensor:
    """An engine tensor [B, H, W, C] → [B, C, H, W] on the host."""
    return t.cpu().permute(0, 3, 1, 2)


def maxpool_ref(x: np.ndarray) -> np.ndarray:
    """3 x 3 / stride 2 / pad 1 maximum of x [B, H, W, C] over in-range pixels only, in x's own dtype."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = None
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            oy0, ox0 = (1 if dy < 0 else 0), (1 if dx < 0 else 0)          # first output whose tap is in range
            oy1 = min(Ho, (H - 1 - dy) // 2 + 1)
            ox1 = min(Wo, (W - 1 - dx) // 2 + 1)
            t = np.full((B, Ho, Wo, C), -np.inf, dtype=x.dtype)
            t[:, oy0:oy1, ox0:ox1] = x[:, 2 * oy0 + dy:2 * (oy1 - 1) + dy + 1:2, 2 * ox0 + dx:2 * (ox1 - 1) + dx + 1:2]
            out = t if out is None else np.maximum(out, t)
    return out


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    ity = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(ity), b.view(ity)))
