"""A checker for td_roi_align with teeth: a float64 reference on the oracle's own sampling geometry, the oracle's float32
result for exact comparison, an error bound, and guarded output buffers (plain module, imported by
tests/test_roi_align_gpu.py; the CPU half runs in the mutation controls of tests/test_roi_ref.py).

Geometry. oracle/ops_ref.py ``roi_align_samples`` (the loop ``roi_align`` itself runs: aligned = True,
sampling_ratio = 0) gives every bin's in-map samples in summation order, with their four corner pixels and float32
weights, and the bin's divisor ``count``. They are flattened once per (RoIs, map size, scale, pooled) into ``Taps``.

Values. Feature values are float32, or fp16 widened to float32; ``gather(y, x)`` returns their rows [n, C].

* ``ref32``: the oracle's float32 arithmetic, ``acc = acc + (((w1 v1 + w2 v2) + w3 v3) + w4 v4)`` sample after sample,
  then ``acc / count``. It is evaluated for all bins at once, sample slot after sample slot, which changes no
  operation and no order: tests/test_roi_ref.py pins it to ``ops_ref.roi_align`` bit for bit.
* ``ref64 = sum (w1 v1 + w2 v2 + w3 v3 + w4 v4) / count`` in float64 (the weights are the float32 ones), and
  ``mag = sum |w v| / count``.

Three checks per launch:

(a) Exactness. The kernels promise the oracle's float32 operation order, so an fp32 output must equal ``ref32`` bit
    for bit and an fp16 output must equal ``float16(ref32)`` (round to nearest even) bit for bit. NaNs must sit where
    the oracle has them (their payload is not compared).
(b) Error bound. Per element with a finite ref64, where ``ghw`` is the bin's divisor (its sample-grid size):
    fp32 ``|got - ref64| <= (4 ghw + 2) 2^-24 mag``; fp16 adds the output rounding ``2^-11 |ref64| + 2^-25``.
(c) Guard zones. The output sits inside one allocation with guards on both sides, all of it prefilled with a
    signalling-NaN pattern no arithmetic produces (tests/conv_ref.py SENTINEL): every element of R * pooled^2 * C
    must be written, and nothing outside it.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle import ops_ref as R
from tests.conv_ref import SENTINEL, Guarded

U32 = 2.0 ** -24
U16 = 2.0 ** -11
GUARD_BYTES = 4 << 10
F32 = np.float32


@dataclasses.dataclass
class Taps:
    """Every in-map sample of every bin, flattened; bins are r * pooled^2 + ph * pooled + pw."""
    nbins: int
    bin: np.ndarray          # [S] int64, non-decreasing
    slot: np.ndarray         # [S] int64, position of the sample in its bin's sum
    yl: np.ndarray
    yh: np.ndarray
    xl: np.ndarray
    xh: np.ndarray
    w: np.ndarray            # [S, 4] float32 (w1, w2, w3, w4)
    count: np.ndarray        # [nbins] float32 divisor

    @property
    def samples(self) -> int:
        return int(self.bin.size)


def taps(rois, H: int, W: int, scale: float, pooled: int) -> Taps:
    rois = np.asarray(rois, dtype=F32).reshape(-1, 4)
    nb = rois.shape[0] * pooled * pooled
    b, s, t, cnt = [], [], [], np.ones(nb, F32)
    for r, ph, pw, count, tp in R.roi_align_samples(rois, H, W, scale, pooled):
        k = (r * pooled + ph) * pooled + pw
        cnt[k] = count
        for i, tap in enumerate(tp):
            b.append(k)
            s.append(i)
            t.append(tap)
    a = np.array([x[:4] for x in t], dtype=np.int64).reshape(-1, 4)
    w = np.array([x[4:] for x in t], dtype=F32).reshape(-1, 4)
    return Taps(nb, np.array(b, np.int64), np.array(s, np.int64), a[:, 0], a[:, 1], a[:, 2], a[:, 3], w, cnt)


def hwc_gather(feat_hwc: np.ndarray):
    """gather(y, x) → rows [n, C] of an [H, W, C] float32 map."""
    f = np.asarray(feat_hwc, dtype=F32)
    return lambda y, x: f[y, x]


def ref32(t: Taps, gather, C: int) -> np.ndarray:
    """The oracle's float32 result [nbins, C] (module docstring)."""
    acc = np.zeros((t.nbins, C), F32)
    if t.samples:
        order = np.argsort(t.slot, kind="stable")
        bounds = np.searchsorted(t.slot[order], np.arange(int(t.slot.max()) + 2))
        for k in range(len(bounds) - 1):
            i = order[bounds[k]:bounds[k + 1]]           # the k-th sample of every bin that has one (bins are distinct)
            w = t.w[i]
            val = (w[:, 0:1] * gather(t.yl[i], t.xl[i]) + w[:, 1:2] * gather(t.yl[i], t.xh[i])
                   + w[:, 2:3] * gather(t.yh[i], t.xl[i]) + w[:, 3:4] * gather(t.yh[i], t.xh[i]))
            b = t.bin[i]
            acc[b] = acc[b] + val
    with np.errstate(invalid="ignore"):
        return acc / t.count[:, None]


def ref64(t: Taps, gather, C: int, chunk_elems: int = 1 << 22):
    """(ref64, mag), both [nbins, C] float64 (module docstring)."""
    s = np.zeros((t.nbins, C))
    m = np.zeros((t.nbins, C))
    step = max(1, chunk_elems // max(C, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, t.samples, step):
            sl = slice(a, min(a + step, t.samples))
            w = t.w[sl].astype(np.float64)
            terms = [w[:, j:j + 1] * gather(yy[sl], xx[sl]).astype(np.float64)
                     for j, (yy, xx) in enumerate(((t.yl, t.xl), (t.yl, t.xh), (t.yh, t.xl), (t.yh, t.xh)))]
            val = terms[0] + terms[1] + terms[2] + terms[3]
            mag = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2]) + np.abs(terms[3])
            b = t.bin[sl]
            starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
            s[b[starts]] += np.add.reduceat(val, starts, axis=0)
            m[b[starts]] += np.add.reduceat(mag, starts, axis=0)
        cnt = t.count.astype(np.float64)[:, None]
        return s / cnt, m / cnt


@dataclasses.dataclass
class Reference:
    r32: np.ndarray          # [nbins, C] float32
    r64: np.ndarray          # [nbins, C] float64
    mag: np.ndarray          # [nbins, C] float64
    ghw: np.ndarray          # [nbins] float64

    def channels(self, C: int) -> "Reference":
        """The first C channels (every channel is computed on its own)."""
        return Reference(self.r32[:, :C], self.r64[:, :C], self.mag[:, :C], self.ghw)


def reference(t: Taps, gather, C: int) -> Reference:
    r64, mag = ref64(t, gather, C)
    return Reference(ref32(t, gather, C), r64, mag, t.count.astype(np.float64))


def new_output(nbins: int, C: int, fp16: bool, device) -> Guarded:
    return Guarded((nbins, C), torch.float16 if fp16 else torch.float32, device, fill=SENTINEL, guard_bytes=GUARD_BYTES)


@dataclasses.dataclass
class Verdict:
    failures: list
    exact: float             # share of elements bit-identical to the oracle
    worst: float             # max |got - ref64| / bound over the finite elements (0 when none)


def _same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    ity = np.int32 if got.dtype == np.float32 else np.int16
    gn, wn = np.isnan(got), np.isnan(want)
    return np.where(gn | wn, gn & wn, got.view(ity) == want.view(ity))


def check(out: Guarded, ref: Reference) -> Verdict:
    fails = []
    if not out.guards_intact():
        fails.append("(c) a guard zone was written")
    unwritten = out.pattern_count()
    if unwritten:
        fails.append(f"(c) {unwritten} output elements left unwritten")
    got = out.t.cpu().numpy()
    fp16 = got.dtype == np.float16
    want = ref.r32.astype(np.float16) if fp16 else ref.r32
    same = _same_bits(got, want)
    if not same.all():
        k = np.argwhere(~same)[0]
        fails.append(f"(a) {int((~same).sum())} of {same.size} elements differ from the oracle; first at (bin, c) = "
                     f"{tuple(int(v) for v in k)}: got {got[tuple(k)]!r}, oracle {want[tuple(k)]!r}")
    fin = np.isfinite(ref.r64) & np.isfinite(ref.mag)
    bound = (4.0 * ref.ghw[:, None] + 2.0) * U32 * ref.mag
    if fp16:
        bound = bound + U16 * np.abs(ref.r64) + 2.0 ** -25
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref.r64)
        bad = fin & ~(err <= bound)
    if bad.any():
        k = np.argwhere(bad)[0]
        fails.append(f"(b) {int(bad.sum())} elements outside the error bound; first at (bin, c) = {tuple(int(v) for v in k)}: "
                     f"got {got[tuple(k)]!r}, ref64 {ref.r64[tuple(k)]!r}, bound {bound[tuple(k)]:.3g}")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    return Verdict(fails, float(same.mean()) if same.size else 1.0, worst)


# ---- cases --------------------------------------------------------------------------------------------------------------
def edge_rois(H: int, W: int, pooled: int) -> np.ndarray:
    """RoIs at scale 1 that reach every edge of the sampling rules on an H x W map."""
    P = float(pooled)
    r = [[0, 0, W, H],                                         # the whole map
         [-10, 5, 12, 30], [5, -10, 30, 12], [W - 12, 5, W + 10, 30], [5, H - 12, 30, H + 10],   # over each border
         [W + 5, H + 5, W + 30, H + 40], [-40, -30, -5, -3],   # entirely outside
         [10, 10, 10, 10], [10, 10, 20, 10],                   # zero area
         [20, 10, 5, 30], [5, 30, 20, 10],                     # inverted
         [10.3, 11.1, 10.55, 11.4], [W - 1.75, H - 1.2, W - 1.5, H - 1.0]]   # sub-pixel
    # exact binary fractions: one-pixel bins (gh = 1) starting at t put samples at t, t + 1, ..., t + pooled - 1 exactly;
    # two-pixel bins (gh = 2) the same with two samples per bin
    for ty in (-1, 0, H - 1, H):
        for tx in (-1, 0, W - 1, W):
            r.append([tx, ty, tx + P, ty + P])
    for t in (-1, H - 1):
        r.append([t, t, t + 2 * P, t + 2 * P])
    return np.array(r, dtype=F32)


def random_rois(rng, n: int, H: int, W: int, scale: float, max_side: float) -> np.ndarray:
    xy = rng.uniform(-0.1, 0.9, (n, 2)) * [W / scale, H / scale]
    wh = rng.uniform(0.05, 1.0, (n, 2)) * (max_side / scale)
    return np.concatenate([xy, xy + wh], axis=1).astype(F32)


def touches_origin(t: Taps, nrois: int, pooled: int) -> np.ndarray:
    """[nrois] bool: the RoI reads pixel (0, 0) through one of its samples' corners (whatever the weight)."""
    hit = ((t.yl == 0) | (t.yh == 0)) & ((t.xl == 0) | (t.xh == 0))
    out = np.zeros(nrois, bool)
    out[np.unique(t.bin[hit] // (pooled * pooled))] = True
    return out
