"""Shared by the resampling tests: the shapes, the seeded rasters, the host results (computed once, read-only) and the float64
evaluation of the separable filter with the SAME float32 weights widened."""
import functools

import numpy as np

from treedetection_amd import postprocessing as P

# name → (rows, cols, out_rows, out_cols). A factor f means (int(rows * f), int(cols * f)), the crown stage's rule; the last two give
# the output shape outright: 7 x 5 → 1 x 1, and 3 x 20 011 at 0.2 along the row — sixteen 256-output workgroup segments, the last one
# with 162 outputs — with its three rows going to one (int(3 * 0.2) is 0, which is no raster).
def _at(h, w, f):
    return h, w, int(h * f), int(w * f)


CASES = {
    "203x317@0.2": _at(203, 317, 0.2),           # → 40 x 63
    "203x317@0.5": _at(203, 317, 0.5),
    "203x317@0.3": _at(203, 317, 0.3),
    "64x64@0.37": _at(64, 64, 0.37),
    "97x131@1.7": _at(97, 131, 1.7),             # → 164 x 222: magnification, two taps, renormalised at the border
    "7x5->1x1": (7, 5, 1, 1),
    "3x20011@0.2": (3, 20011, 1, int(20011 * 0.2)),
}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def u8_raster(name):
    """Random four-band uint8 raster [4, rows, cols] of the case."""
    h, w = CASES[name][:2]
    return _frozen(np.random.default_rng(sorted(CASES).index(name) + 100).integers(0, 256, (4, h, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def f32_raster(name):
    """Single-band normal(10, 8) float32 raster [1, rows, cols] of the case."""
    h, w = CASES[name][:2]
    return _frozen(np.random.default_rng(sorted(CASES).index(name) + 200).normal(10.0, 8.0, (1, h, w)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def host_u8(name):
    """postprocessing.resample_bilinear_gdal of the uint8 raster: [4, out_rows, out_cols] uint8."""
    return _frozen(P.resample_bilinear_gdal(u8_raster(name), *CASES[name][2:]))


def eval64(arr, out_h, out_w):
    """The separable filter in float64 with the float32 weights widened: [bands, out_h, out_w] float64, not rounded."""
    bands, h, w = arr.shape
    work = arr.astype(np.float64)
    tmp = np.empty((bands, h, out_w), np.float64)
    for j, (idx, wgt) in enumerate(P._decimation_weights(w, out_w)):
        tmp[:, :, j] = work[:, :, idx] @ wgt.astype(np.float32).astype(np.float64)
    out = np.empty((bands, out_h, out_w), np.float64)
    for i, (idx, wgt) in enumerate(P._decimation_weights(h, out_h)):
        out[:, i, :] = np.tensordot(wgt.astype(np.float32).astype(np.float64), tmp[:, idx, :], axes=([0], [1]))
    return out


@functools.lru_cache(maxsize=None)
def eval64_u8(name):
    return _frozen(eval64(u8_raster(name), *CASES[name][2:]))


@functools.lru_cache(maxsize=None)
def eval64_f32(name):
    return _frozen(eval64(f32_raster(name), *CASES[name][2:]))


def f32_bound(h, w, out_h, out_w, max_abs):
    """First-order error bound of the two sequential float32 sums (non-negative weights that sum to one) against the float64
    evaluation: (nx + ny + 4) * 2^-24 * max|src|, nx / ny the largest tap counts of the two axes."""
    nx = max(len(idx) for idx, _ in P._decimation_weights(w, out_w))
    ny = max(len(idx) for idx, _ in P._decimation_weights(h, out_h))
    return (nx + ny + 4) * 2.0 ** -24 * float(max_abs)
