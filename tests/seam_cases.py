"""Shared by tests/test_seam_windows.py (CPU) and tests/test_seam_gpu.py: the raster windows both put through the windowed block plan /
decode, the geometry cases of the seam strips, and the strip rule restated in numpy on ``merging._equals``."""
import numpy as np

from treedetection_amd.merging import _equals


def windows(H, W, bh, bw):
    """(r0, c0, h, w) windows of an H x W raster in bh x bw blocks (strips: bw = W) → {name: window}: one pixel, one whole block, one
    that starts mid-block, one that ends in the last rows and columns (the short last strip, the partly filled last block column),
    the top-left corner block, and the whole raster."""
    by, bx = min(1, (H - 1) // bh), min(1, (W - 1) // bw)
    return {
        "pixel": (min(bh + 2, H - 1), min(bw + 3, W - 1), 1, 1),
        "block": (by * bh, bx * bw, min(bh, H - by * bh), min(bw, W - bx * bw)),
        "midblock": (bh // 2 + 1, bw // 2 + 1, min(bh, H - bh // 2 - 1), min(bw, W - bw // 2 - 1)),
        "end": (H - 3, W - 5, 3, 5),
        "corner": (0, 0, min(bh, H), min(bw, W)),
        "whole": (0, 0, H, W),
    }


# tests/test_merging.py's geometry cases: dtype, bands, (h1, w1), (h2, w2), offset of raster 2 in pixels (dx, dy), nodata tag of
# raster 1, zero fraction — adjacent, overlapping, negative offset, unequal sizes
GEOMETRY = [
    (np.uint8, 4, (40, 50), (40, 50), (50, 0), None, 0.0),
    (np.uint8, 4, (40, 50), (40, 50), (0, 40), None, 0.0),
    (np.float32, 1, (30, 30), (30, 30), (30, 0), None, 0.0),
    (np.uint8, 3, (40, 50), (40, 50), (35, 0), None, 0.3),
    (np.uint8, 3, (40, 50), (30, 60), (-20, 25), None, 0.3),
    (np.float32, 1, (32, 32), (32, 32), (16, 16), -9999.0, 0.2),
    (np.float32, 1, (32, 32), (32, 32), (16, 0), 3.4e38, 0.2),
    (np.uint16, 2, (20, 25), (20, 25), (10, 5), None, 0.5),
]


def rand_raster(rng, bands, h, w, dtype, zero_frac=0.0):
    if np.issubdtype(np.dtype(dtype), np.integer):
        a = rng.integers(1, 250, (bands, h, w)).astype(dtype)
    else:
        a = rng.uniform(0.5, 40.0, (bands, h, w)).astype(dtype)
    if zero_frac:
        a[:, rng.random((h, w)) < zero_frac] = 0
    return a


def first_rule(strip, fill, parts):
    """The strip rule, sample by sample as numpy evaluates it: ``strip`` [rows, cols, bands] starts at ``fill``; every part (source
    pixels [h, w, bands], (row, col) of its first pixel in the strip, own nodata or None) in turn is copied where the strip still
    equals ``fill`` and the source sample is not its own nodata. In place; → strip."""
    strip[...] = fill
    for new, (r, c), own in parts:
        view = strip[r:r + new.shape[0], c:c + new.shape[1]]
        free = _equals(view, fill)
        if own is not None:
            free &= ~_equals(new, own)
        np.copyto(view, new, where=free)
    return strip
