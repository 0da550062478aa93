"""A checker for td_conv2d_nhwc with teeth: guarded buffers, seeded device inputs, a sampled float64 reference and an
error bound that holds for any summation order (plain module, imported by the conv tests; the CPU half runs in the
mutation controls of tests/test_conv_ref.py).

Buffers. The output y sits inside one larger allocation with GUARD_BYTES on each side; the whole allocation is filled
with a signalling-NaN bit pattern (fp32 0x7FA5A5A5, fp16 0x7D5A) that no arithmetic produces. After a launch both guards
must still hold the pattern byte for byte (no write past either end) and no element of y may hold it (no row left
unwritten). Inputs (x, residual) sit inside allocations filled with quiet NaN: a read outside a tensor that feeds a
stored output turns that output into NaN. All checks are torch ops on the tensors' device; only counts and the sampled
rows reach the host.

Launches with a device row count (td_conv2d_rows_nhwc; the mask head): `check(..., live_rows=n)` compares only conv rows
below n, and every element of y that belongs to a row at or past n must still hold the sentinel. With out_mode 1 (the 2x2
deconvolution's pixel-shuffle store) the reference is laid out as y is stored: y[b, 2h+dy, 2w+dx, co] comes from filter row
(dy*2+dx)*Cq + co of conv row (b, h, w), with the scale and bias of co.

Reference. For a sample of output pixels (every image's corners, the borders of a few images, the first and last row
of 256-row M blocks at the start, middle and end, the whole ragged last M tile, and >= 2048 seeded random pixels; every
output channel of each), the input patches are gathered on the device and converted to float64 on the host:

    y64 = act(patch @ W64^T * scale + bias [+ residual, nearest-2x when res_shift]),   S = |patch| @ |W|^T

Per-element bound (never a false failure). With u = 2^-24, gamma_K = 1.05 K u (>= K u / (1 - K u) for K u < 0.04) and
A = |scale| S (1 + gamma_K) + |bias| + |residual| (a bound on every intermediate of the epilogue):

    |y - y64| <= gamma_K |scale| S  +  4 u A  [ + 2^-11 (|y64| + gamma_K |scale| S + 4 u A) + 2^-25  for fp16 outputs ]

The first term is the classical bound of a K-term fp32 dot product in ANY summation order (fp16 products are exact in
fp32, so there only the sums round); the second covers the epilogue's scale, bias and residual roundings (one u each,
with room); the third is the final rounding of an fp16 output.

Statistical criterion. The bound above is loose by about sqrt(K): at K ~ 2304 a tile that stages partial sums in fp16
stays inside it. So the sample also has to pass an RMS test. Each element gets the error scale of fp32 accumulation
(a random walk of K roundings of the running sum), plus its output rounding:

    n^2 = (u |scale| Q sqrt(K))^2 + (u A)^2 + (u_out |y64|)^2,   Q = sqrt(sum_k (a_k w_k)^2),   u_out = 2^-11 (fp16) or 0

    R = sqrt(sum (y - y64)^2 / sum n^2)  <=  RMS_MAX[output dtype]

RMS_MAX was fitted on an MI355X (every tile of tests/test_conv_shapes_gpu.py, every shape, precision and batch there);
the worst R measured was RMS_WORST_MEASURED (fp32 outputs 0.339, fp16 outputs 0.427; every tile gave the same values,
they keep one k order), and RMS_MAX (1.4 / 1.75) leaves a margin of at least 4x over it. An emulated tile that holds its
accumulator in fp16 measures R = 2.7 at K = 2304 (test_conv_ref.py), rejected by this criterion alone.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -11
GUARD_BYTES = 64 << 10
BLOCK_ROWS = 256
# signalling-NaN sentinels (quiet bit clear) and the quiet NaN the inputs are wrapped in, as (int view dtype, bit pattern)
SENTINEL = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.float16: (torch.int16, 0x7D5A)}
QNAN = {torch.float32: (torch.int32, 0x7FC00000), torch.float16: (torch.int16, 0x7E00)}
# per output dtype, fitted on the MI355X sweep (see the module docstring): fp32 worst 0.339 (box predictor, K = 1024, where
# the epilogue roundings dominate), fp16 worst 0.427 (the output rounding); RMS_MAX = 4.1x each
RMS_WORST_MEASURED = {torch.float32: 0.339, torch.float16: 0.427}
RMS_MAX = {torch.float32: 1.4, torch.float16: 1.75}


class Guarded:
    """A tensor of `shape` inside one allocation with `guard_bytes` of `fill` (SENTINEL / QNAN) on each side."""

    def __init__(self, shape, dtype, device, fill=SENTINEL, guard_bytes=GUARD_BYTES):
        es = torch.empty((), dtype=dtype).element_size()
        self.n = int(np.prod(shape))
        self.g = guard_bytes // es
        self.ity, self.pattern = fill[dtype]
        self.buf = torch.empty(self.g + self.n + self.g, dtype=dtype, device=device)
        self.buf.view(self.ity).fill_(self.pattern)
        self.t = self.buf[self.g:self.g + self.n].view(shape)

    def data_ptr(self):
        return self.t.data_ptr()

    def guards_intact(self) -> bool:
        b = self.buf.view(self.ity)
        return bool((b[:self.g] == self.pattern).all().item() and (b[self.g + self.n:] == self.pattern).all().item())

    def pattern_count(self) -> int:
        return int((self.t.reshape(-1).view(self.ity) == self.pattern).sum().item())


@dataclasses.dataclass(frozen=True)
class Conv:
    """One convolution launch: x [B,H,W,Cin] -> y [B,Ho,Wo,Cout]; res 0 none / 1 same size / 2 nearest-2x upsampled.
    out_mode 1 (the 2x2 deconvolution as a 1x1 layer with a pixel-shuffle store): y [B,2Ho,2Wo,Cq], Cq = Cout/4, filter
    row (dy*2+dx)*Cq + co lands at y[b, 2h+dy, 2w+dx, co]; scale and bias have Cq entries."""
    name: str
    Cin: int
    Cout: int
    k: int
    stride: int
    pad: int
    H: int
    W: int
    scale: bool = True
    bias: bool = True
    res: int = 0
    relu: bool = True
    out_f32: bool = False
    out_mode: int = 0

    @property
    def Ho(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pad - self.k) // self.stride + 1

    @property
    def K(self):
        return self.k * self.k * self.Cin

    @property
    def Cy(self):
        """Channels of a pixel of y as stored."""
        return self.Cout // 4 if self.out_mode == 1 else self.Cout

    @property
    def y_shape(self):
        """(rows, columns) of one image of y as stored."""
        return (2 * self.Ho, 2 * self.Wo) if self.out_mode == 1 else (self.Ho, self.Wo)


def make_inputs(L: Conv, fp16: bool, B: int, device, seed: int) -> dict:
    """Seeded inputs generated on `device` (fp16 tensors are generated as fp16: the reference reads the kernel's bits).
    Activations: |N(0,1)| with ~15% exact zeros (post-ReLU maps); weights N(0, 1/K); per-channel scale U(0.5,1.5), bias N(0,0.5)."""
    dt = torch.float16 if fp16 else torch.float32
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    x = Guarded((B, L.H, L.W, L.Cin), dt, device, fill=QNAN)
    torch.randn(x.t.shape, generator=g, dtype=dt, device=device, out=x.t)
    x.t.abs_()
    x.t.mul_((torch.rand(x.t.shape, generator=g, dtype=dt, device=device) > 0.15).to(dt))
    w = torch.randn((L.Cout, L.k, L.k, L.Cin), generator=g, dtype=torch.float32, device=device).mul_(1.0 / math.sqrt(L.K)).to(dt)
    scale = torch.rand(L.Cy, generator=g, device=device).add_(0.5) if L.scale else None
    bias = torch.randn(L.Cy, generator=g, device=device).mul_(0.5) if L.bias else None
    res = None
    if L.res:
        sh = (B, L.Ho, L.Wo, L.Cout) if L.res == 1 else (B, L.Ho >> 1, L.Wo >> 1, L.Cout)
        res = Guarded(sh, dt, device, fill=QNAN)
        torch.randn(sh, generator=g, dtype=dt, device=device, out=res.t)
    return dict(x=x, w=w, scale=scale, bias=bias, res=res, B=B, fp16=fp16)


def out_dtype(L: Conv, fp16: bool):
    return torch.float16 if fp16 and not L.out_f32 else torch.float32


def new_output(L: Conv, inp: dict) -> Guarded:
    return Guarded((inp["B"],) + L.y_shape + (L.Cy,), out_dtype(L, inp["fp16"]), inp["x"].t.device)


def launch(L: Conv, inp: dict, y: Guarded, tile_cfg: int = -1, strict: bool = True, B: int = None, W: int = None, H: int = None,
           count: torch.Tensor = None, rows_mul: int = None, rows_entry: bool = False):
    """td_conv2d_nhwc on the guarded buffers (B / H / W override the map size: the 4 GB refusal). Raises on a refused launch.
    `count` (a device int32 scalar: the kernels compute min(M, count * rows_mul) rows; rows_mul defaults to Ho * Wo, a count
    of images), an out_mode 1 layer or `rows_entry` go through td_conv2d_rows_nhwc (stride 1, no residual)."""
    from treedetection_amd import _lib
    from tests.gpu_util import STRICT
    lib = _lib.load()
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    prec = (1 if inp["fp16"] else 0) | ((tile_cfg + 1) << 8) | (0x10000 if L.out_f32 else 0) | (STRICT if strict else 0)
    if count is not None or L.out_mode or rows_entry:
        assert L.stride == 1 and not L.res and (count is None or (count.dtype == torch.int32 and count.is_cuda and count.numel() == 1))
        st = lib.td_conv2d_rows_nhwc(p(inp["x"]), p(inp["w"]), p(inp["scale"]), p(inp["bias"]), p(y), B or inp["B"], H or L.H, W or L.W,
                                     L.Cin, L.Cout, L.k, L.k, L.pad, int(L.relu), L.out_mode, p(count),
                                     (rows_mul or L.Ho * L.Wo) if count is not None else 1, prec, _lib.stream_ptr())
        _lib.check(st, "td_conv2d_rows_nhwc")
        return
    st = lib.td_conv2d_nhwc(p(inp["x"]), p(inp["w"]), p(inp["scale"]), p(inp["bias"]), p(inp["res"]), 1 if L.res == 2 else 0, p(y),
                            B or inp["B"], H or L.H, W or L.W, L.Cin, L.Cout, L.k, L.k, L.stride, L.pad, int(L.relu), prec,
                            _lib.stream_ptr())
    _lib.check(st, "td_conv2d_nhwc")


def sample_rows(L: Conv, B: int, seed: int, n_random: int = 2048, tail: int = 0) -> torch.Tensor:
    """Output rows (pixel indices b*Ho*Wo + oh*Wo + ow) to check; all channels of each are compared. `tail` > 0 puts
    the random sample in the last `tail` rows instead of the whole map (the 4 GB cases)."""
    Ho, Wo = L.Ho, L.Wo
    HW, M = Ho * Wo, B * Ho * Wo
    rng = np.random.default_rng(seed)
    rows = []
    imgs = np.arange(B) if B <= 64 else np.unique(np.concatenate([[0, B - 1], rng.integers(0, B, 62)]))
    for b in imgs:                                                     # corners (padding taps on two sides)
        rows += [b * HW, b * HW + Wo - 1, b * HW + (Ho - 1) * Wo, b * HW + HW - 1]
    bimgs = np.unique(np.concatenate([[0, B - 1], rng.integers(0, B, 2)]))
    for b in bimgs:                                                    # whole borders of a few images (strided on big maps)
        sw, sh = max(1, Wo // 64), max(1, Ho // 64)
        for ow in range(0, Wo, sw):
            rows += [b * HW + ow, b * HW + (Ho - 1) * Wo + ow]
        for oh in range(0, Ho, sh):
            rows += [b * HW + oh * Wo, b * HW + oh * Wo + Wo - 1]
    nb = -(-M // BLOCK_ROWS)
    for blk in {0, 1, 2, nb // 2 - 1, nb // 2, nb - 2, nb - 1}:        # first / last row of blocks at the start, middle, end
        if 0 <= blk < nb:
            rows += [blk * BLOCK_ROWS, min(M, (blk + 1) * BLOCK_ROWS) - 1]
    last = (nb - 1) * BLOCK_ROWS                                       # the whole ragged (or full) last M tile
    rows += list(range(last, M))
    lo = max(0, M - tail) if tail else 0
    rows += list(rng.integers(lo, M, n_random))
    r = np.unique(np.asarray(rows, dtype=np.int64))
    return torch.from_numpy(r[(r >= 0) & (r < M)])


def _patches(L: Conv, x: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """[S, KH*KW*Cin] input patches of the sampled output rows (zeros for padding taps), gathered on x's device."""
    dev = x.device
    B, H, W, Cin = x.shape
    r = rows.to(dev)
    b, rem = r // (L.Ho * L.Wo), r % (L.Ho * L.Wo)
    oh, ow = rem // L.Wo, rem % L.Wo
    kk = torch.arange(L.k, device=dev)
    ih = (oh * L.stride - L.pad)[:, None, None] + kk[None, :, None]
    iw = (ow * L.stride - L.pad)[:, None, None] + kk[None, None, :]
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    idx = (b[:, None, None] * H + ih.clamp(0, H - 1)) * W + iw.clamp(0, W - 1)
    p = x.reshape(-1, Cin)[idx.reshape(-1)].reshape(len(r), L.k * L.k, Cin)
    p = torch.where(ok.reshape(len(r), L.k * L.k, 1), p, torch.zeros((), dtype=p.dtype, device=dev))
    return p.reshape(len(r), -1)


def _residual_rows(L: Conv, res: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    r = rows.to(res.device)
    if L.res == 1:
        return res.reshape(-1, L.Cout)[r]
    b, rem = r // (L.Ho * L.Wo), r % (L.Ho * L.Wo)
    oh, ow = rem // L.Wo, rem % L.Wo
    Hr, Wr = res.shape[1], res.shape[2]
    return res.reshape(-1, L.Cout)[(b * Hr + (oh >> 1)) * Wr + (ow >> 1)]


@dataclasses.dataclass
class Reference:
    rows: torch.Tensor       # pixel indices of y AS STORED (out_mode 0: the conv rows; out_mode 1: four shuffled pixels per conv row)
    y64: torch.Tensor        # [S, Cy] float64 (host)
    bound: torch.Tensor      # per-element bound
    norm2: torch.Tensor      # per-element RMS normaliser squared
    A: torch.Tensor          # |scale| S (1 + gamma_K) + |bias| + |residual| (the Winograd bound's scale)


def stored_rows(L: Conv, rows: torch.Tensor) -> torch.Tensor:
    """Pixel indices of y as stored for conv rows `rows`: [S] for out_mode 0, [S, 4] (q = dy*2+dx) for the pixel shuffle."""
    if L.out_mode != 1:
        return rows
    b, rem = rows // (L.Ho * L.Wo), rows % (L.Ho * L.Wo)
    h, w = rem // L.Wo, rem % L.Wo
    q = torch.arange(4)
    return (b[:, None] * 2 * L.Ho + 2 * h[:, None] + (q >> 1)[None]) * (2 * L.Wo) + 2 * w[:, None] + (q & 1)[None]


def conv_row_of_pixel(L: Conv, px: torch.Tensor) -> torch.Tensor:
    """The conv row that writes pixel `px` of y as stored (the inverse of stored_rows)."""
    if L.out_mode != 1:
        return px
    H2, W2 = L.y_shape
    b, rem = px // (H2 * W2), px % (H2 * W2)
    return (b * L.Ho + (rem // W2) // 2) * L.Wo + (rem % W2) // 2


def reference(L: Conv, inp: dict, rows: torch.Tensor) -> Reference:
    """The sampled float64 reference, its per-element bound and RMS normaliser (see the module docstring). `rows` are conv
    rows; with out_mode 1 filter row n = (dy*2+dx)*Cq + co of conv row (b,h,w) is y[b, 2h+dy, 2w+dx, co], with scale / bias of co."""
    P = _patches(L, inp["x"].t, rows).cpu().double()
    Wm = inp["w"].reshape(L.Cout, -1).cpu().double()
    y0 = P @ Wm.T
    S = P.abs() @ Wm.abs().T
    Q = ((P * P) @ (Wm * Wm).T).sqrt()
    sc = inp["scale"].cpu().double() if inp["scale"] is not None else torch.ones(L.Cy, dtype=torch.float64)
    bi = inp["bias"].cpu().double() if inp["bias"] is not None else torch.zeros(L.Cy, dtype=torch.float64)
    if L.out_mode == 1:                                                        # n = q*Cq + co takes the scale / bias of co
        sc, bi = sc.repeat(4), bi.repeat(4)
    rr = _residual_rows(L, inp["res"].t, rows).cpu().double() if inp["res"] is not None else torch.zeros_like(y0)
    y = y0 * sc + bi + rr
    if L.relu:
        y = y.clamp_min(0)
    gamma = 1.05 * L.K * U32
    A = sc.abs() * S * (1 + gamma) + bi.abs() + rr.abs()
    bound = gamma * sc.abs() * S + 4 * U32 * A
    uo = U16 if out_dtype(L, inp["fp16"]) == torch.float16 else 0.0
    bound = bound + (uo * (y.abs() + bound) + 2.0 ** -25 if uo else 0.0)       # (+ half the fp16 subnormal spacing)
    norm2 = (U32 * sc.abs() * Q * math.sqrt(L.K)) ** 2 + (U32 * A) ** 2 + (uo * y) ** 2
    sh = lambda t: t.reshape(-1, L.Cy)                                         # noqa: E731  ([S, 4*Cq] -> [4S, Cq], q-major per row)
    return Reference(stored_rows(L, rows).reshape(-1), sh(y), sh(bound), sh(norm2), sh(A))


@dataclasses.dataclass
class Verdict:
    ok: bool
    why: str
    err_over_bound: float
    rms: float


def check(L: Conv, y: Guarded, ref: Reference, live_rows: int = None) -> Verdict:
    """Guards, leftover sentinel, finiteness, the per-element bound and the RMS criterion for one launch's output.
    `live_rows` (a launch with a device row count): only conv rows below it are compared, none of their elements may hold
    the sentinel, and EVERY element of y that belongs to a conv row at or past it must still hold the sentinel bit pattern."""
    if not y.guards_intact():
        return Verdict(False, "a guard zone around y was written", math.inf, math.inf)
    C = L.Cy
    flat = y.t.reshape(-1, C)
    dev = flat.device
    is_pat = flat.view(y.ity) == y.pattern
    keep = None
    if live_rows is None:
        left, live_vals = int(is_pat.sum().item()), flat
    else:
        live = conv_row_of_pixel(L, torch.arange(flat.shape[0], device=dev)) < live_rows
        touched = (~is_pat).any(1) & ~live
        if bool(touched.any().item()):
            bad = touched.nonzero()[:8, 0].tolist()
            return Verdict(False, f"{int(touched.sum())} pixels of y at or past the row count ({live_rows} rows) were written: pixels {bad}",
                           math.inf, math.inf)
        left, live_vals = int((is_pat & live[:, None]).sum().item()), flat[live]
        keep = live[ref.rows.to(dev)].cpu()
    if left:
        return Verdict(False, f"{left} elements of y were never written (sentinel left)", math.inf, math.inf)
    if not bool(torch.isfinite(live_vals).all().item()):
        bad = (~torch.isfinite(flat)).any(1).nonzero()[:8, 0].tolist()
        return Verdict(False, f"non-finite outputs at rows {bad}", math.inf, math.inf)
    rows, y64, bnd, norm2 = ref.rows, ref.y64, ref.bound, ref.norm2
    if keep is not None:
        rows, y64, bnd, norm2 = rows[keep], y64[keep], bnd[keep], norm2[keep]
    if len(rows) == 0:
        return Verdict(True, "", 0.0, 0.0)
    got = flat[rows.to(dev)].cpu().double()
    err = (got - y64).abs()
    ratio = err / bnd.clamp_min(1e-300)
    worst = float(ratio.max())
    rms = math.sqrt(float((err * err).sum()) / max(float(norm2.sum()), 1e-300))
    if worst > 1.0:
        i = int(ratio.argmax())
        r, c = int(rows[i // C]), i % C
        n = int((ratio > 1).sum())
        return Verdict(False, f"{n} sampled outputs over the fp64 bound; worst err/bound {worst:.3g} at row {r} channel {c} "
                              f"(got {float(got.reshape(-1)[i]):.9g}, fp64 {float(y64.reshape(-1)[i]):.9g})", worst, rms)
    if rms > RMS_MAX[y.t.dtype]:
        return Verdict(False, f"RMS error {rms:.3g} x the fp32-accumulation scale > RMS_MAX {RMS_MAX[y.t.dtype]}", worst, rms)
    return Verdict(True, "", worst, rms)


# ---- which tile ids a launch accepts, and which the engine's tuner times (mirrors conv2d_launch and tuned_cfg) ----
SWEEP_IDS = [c for c in range(34) if c not in (21, 22, 28)]      # 21 / 22 / 28: retired experiments, always refused
TUNE_CANDIDATES = [33, 10, 17, 29, 16, 0, 15, 30, 23, 27, 1, 2, 24, 25, 26, 31, 3, 32, 18, 19, 20]   # common.h
_LIM = 0xFFFFFFF0 - (1 << 20)


def _plane_ok(L: Conv, fp16: bool, B: int) -> bool:
    return (not fp16 and L.k == 1 and L.stride == 1 and L.pad == 0 and L.res != 2 and not L.out_f32 and L.Cin % 32 == 0
            and B * L.Ho * L.Wo * L.Cin * 4 < _LIM)


def _bs_ok(L: Conv, fp16: bool, B: int) -> bool:
    es = 2 if fp16 else 4
    nit = L.Cin // (128 // es)
    M = B * L.Ho * L.Wo
    return (L.k == 1 and L.stride == 1 and L.pad == 0 and not L.out_f32 and L.Cin % (128 // es) == 0 and nit in (1, 2, 4)
            and 128 <= L.Cout <= 2048 and L.Cout % 8 == 0 and M * L.Cin * es < _LIM and M * L.Cout * es < _LIM)


def _bd_ok(L: Conv, fp16: bool) -> bool:
    ke = 64 if fp16 else 32
    return L.Cin % ke == 0 and L.k * L.k <= 32 and -(-L.Cout // 32) * L.k * L.k * (L.Cin // ke) * 4096 < _LIM


def tile_runs(cfg: int, L: Conv, fp16: bool, B: int, dyn: bool = False) -> bool:
    """Whether td_conv2d_nhwc / td_conv2d_rows_nhwc in strict mode runs tile `cfg` on this launch (conv_tile_refusal's rules;
    `dyn`: the launch carries a device row count). The fp16 ping-pong tile, the plane tiles and the filter-direct family
    store plain rows only (no out_mode 1); the filter-stationary tile takes neither out_mode 1 nor a device count."""
    if cfg in (21, 22, 28) or not 0 <= cfg <= 33:
        return False
    if cfg == 17:
        return fp16 and L.out_mode == 0
    if 18 <= cfg <= 20:
        return _plane_ok(L, fp16, B) and L.out_mode == 0
    if cfg == 33:
        return _bs_ok(L, fp16, B) and L.out_mode == 0 and not dyn
    if 23 <= cfg <= 27 or cfg in (29, 30):
        return _bd_ok(L, fp16) and L.out_mode == 0
    return True


def tuner_ids(L: Conv, fp16: bool, B: int, dyn: bool = False) -> list:
    """The ids the engine's tuned_cfg times for this layer shape (engine.cpp: the direct-conv candidates of one layer with
    a fragment-ordered filter copy — every engine layer whose Cin is a multiple of the k-chunk has one). A candidate that
    conv_tile_refusal refuses for the launch's out_mode or device row count (`dyn`) is never timed."""
    ksteps = L.K // (64 if fp16 else 32)
    plane = _plane_ok(L, fp16, B)
    bd = L.Cin % (64 if fp16 else 32) == 0 and L.k * L.k <= 32
    out = []
    for c in TUNE_CANDIDATES:
        if 14 <= c <= 16 and ksteps > 4:
            continue
        if c == 17 and not (fp16 and L.Cout >= 128):
            continue
        if 18 <= c <= 20 and not plane:
            continue
        if (23 <= c <= 27 or c in (29, 30, 33)) and not bd:
            continue
        if c == 33 and not (L.k == 1 and L.stride == 1 and L.Cout >= 128 and ksteps <= 4 and ksteps != 3):
            continue
        if c in (31, 32) and L.Cout > 32:
            continue
        if L.out_mode != 0 and (c == 17 or 18 <= c <= 20 or 23 <= c <= 27 or c in (29, 30, 33)):
            continue
        if dyn and c == 33:
            continue
        out.append(c)
    return out
