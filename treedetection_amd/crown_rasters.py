"""Crowns against rasters, for postprocessing.process_layer and write_crown_raster: per-crown statistics over the reference's bounding
circles (``td_crown_stats``: a workgroup per crown over its circle's bounding box, the reference's membership arithmetic) or over the
pixels inside each OUTLINE (``td_crown_zonal_dev``, a wave per crown), and label rasters drawn from the outlines (``td_crown_labels_dev``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .crown_device import check_raster_tensor, nonempty, pack_rings, take_rings, upload_rings


def _window(t, n_rows, n_cols, bounds) -> Tuple[int, int, int, int]:
    """The reference's subset of a raster for ``bounds`` (postprocessing.py:45-57; its row / col names are swapped
    twice and cancel): (row_lo, col_lo, row_hi, col_hi)."""
    minx, miny, maxx, maxy = bounds
    if t[0] == 0 or t[4] == 0:
        raise ValueError(f"Affine transform scaling factors are zero: {t[0]}, {t[4]}")
    r_a, c_a = int((miny - t[5]) / t[4]), int((minx - t[2]) / t[0])     # utilities.geo_to_raster: truncation toward zero
    r_b, c_b = int((maxy - t[5]) / t[4]), int((maxx - t[2]) / t[0])
    c_lo, c_hi = sorted([min(c_a, n_cols - 1), max(c_b, 0)])
    r_lo, r_hi = sorted([min(r_a, n_rows - 1), max(r_b, 0)])
    return r_lo, c_lo, r_hi, c_hi


def crown_circles(rings: Sequence[np.ndarray]) -> np.ndarray:
    """[n,3] float32 (cx, cy, r): centre of the bounding box of the float32 vertex coordinates and the largest vertex
    distance from it (postprocessing.py:79-95)."""
    out = np.zeros((len(rings), 3), np.float32)
    for i, r in enumerate(rings):
        x, y = r[:, 0].astype(np.float32), r[:, 1].astype(np.float32)
        cx = (x.min() + x.max()) / np.float32(2)
        cy = (y.min() + y.max()) / np.float32(2)
        dx, dy = x - cx, y - cy
        out[i] = (cx, cy, np.sqrt(dx ** 2 + dy ** 2).max())
    return out


def crown_stats(raster, transform, bounds, circles: np.ndarray, mode: int, radius_scale: float = 1.0,
                device: int = 0, clamp_shape: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """td_crown_stats over one raster → [n,3] (mode 0: max height, x, y) or [n,4] (mode 1: NDVI min, max, mean, var).
    ``raster``: a numpy array [rows, cols] (copied to ``device``), or a contiguous float32 CUDA tensor [rows, cols] (a raster
    decoded in HBM, GeoTiff.decode_to_device), which the kernel reads where it lies."""
    n = circles.shape[0]
    cols_out = 3 if mode == 0 else 4
    if n == 0:
        return np.zeros((0, cols_out), np.float32)
    check_raster_tensor(raster, "crown_stats")
    on_device = isinstance(raster, torch.Tensor)
    rows, cols = raster.shape
    cr, cc = clamp_shape if clamp_shape else (rows, cols)
    r_lo, c_lo, r_hi, c_hi = _window(transform, cr, cc, bounds)
    r_hi, c_hi = min(r_hi, rows - 1), min(c_hi, cols - 1)
    lib = _lib.load()
    dev = raster.device if on_device else torch.device("cuda", device)
    d_r = raster if on_device else torch.from_numpy(np.ascontiguousarray(raster, dtype=np.float32)).to(dev)
    d_c = torch.from_numpy(np.ascontiguousarray(circles, dtype=np.float32)).to(dev)
    d_o = torch.empty((n, cols_out), dtype=torch.float32, device=dev)
    win = (C.c_int32 * 4)(r_lo, c_lo, r_hi, c_hi)
    with torch.cuda.device(dev):
        _lib.check(lib.td_crown_stats(d_r.data_ptr(), rows, cols, _lib.transform6(transform), win, d_c.data_ptr(), n, mode, float(radius_scale),
                                      d_o.data_ptr(), _lib.stream_ptr()), "td_crown_stats")
    return d_o.cpu().numpy()


# ---- zonal statistics over the crown outlines (opt-in: ``crown_statistics: polygon``) ------------------------------------------
def _zonal_host(raster, transform, xy: np.ndarray, start: np.ndarray):
    """td_crown_zonal on host arrays (a raster tensor is downloaded) → (out float32 [n, 4], pos int32 [n, 3], status int32 [n])."""
    n = start.size - 1
    out, pos, status = np.empty((n, 4), np.float32), np.empty((n, 3), np.int32), np.empty(n, np.int32)
    r = np.ascontiguousarray(raster.cpu().numpy() if isinstance(raster, torch.Tensor) else raster, dtype=np.float32)
    _lib.check(_lib.load().td_crown_zonal(r.ctypes.data, r.shape[0], r.shape[1], _lib.transform6(transform), nonempty(xy).ctypes.data, xy.shape[0],
                                          start.ctypes.data, n, out.ctypes.data, pos.ctypes.data, status.ctypes.data), "td_crown_zonal")
    return out, pos, status


def crown_zonal_stats(raster, transform, rings, device: Optional[int] = 0, packed=None, uploaded=None):
    """Zonal statistics of one raster over crown outlines → (stats float32 [n, 4] = min, max, mean, population variance; count
    int32 [n]; max_pos int32 [n, 2] = raster row, column of the maximum; status int32 [n]). A pixel belongs to a crown when its
    centre lies inside the closed ring or on it (include/treedet.h, td_crown_zonal). ``raster``: a numpy array [rows, cols]
    (copied to ``device``), or a contiguous float32 CUDA tensor, which the kernel reads where it lies. ``rings``: [m, 2] vertex
    arrays, closed or open, either winding. ``device``: a GPU index (td_crown_zonal_dev, a wave per crown) or None (td_crown_zonal
    on the host: the same status, count, min, max and position). Crowns the kernel leaves out (status 1: more than
    ``_lib.ZONAL_RING_CAP`` vertices) are decided by the host function alone and merged, status included. Refused crowns
    (status 2: fewer than 3 vertices, a non-finite coordinate) come back as NaN / -1. ``packed`` = pack_rings(rings) and
    ``uploaded`` = upload_rings(*packed, dev), when the caller has them already (two rasters, one ring set)."""
    check_raster_tensor(raster, "crown_zonal_stats")
    xy, start = packed if packed is not None else pack_rings(rings)
    n = start.size - 1
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    on_device = isinstance(raster, torch.Tensor)
    if device is None:
        out, pos, status = _zonal_host(raster, transform, xy, start)
        return out, pos[:, 0].copy(), pos[:, 1:].copy(), status
    rows, cols = raster.shape
    dev = raster.device if on_device else torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_r = raster if on_device else torch.from_numpy(np.ascontiguousarray(raster, dtype=np.float32)).to(dev)
        d_xy, d_start = uploaded if uploaded is not None else upload_rings(xy, start, dev)
        d_o = torch.empty((n, 4), dtype=torch.float32, device=dev)
        d_p = torch.empty((n, 3), dtype=torch.int32, device=dev)
        d_s = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().td_crown_zonal_dev(d_r.data_ptr(), rows, cols, _lib.transform6(transform), d_xy.data_ptr(), xy.shape[0], d_start.data_ptr(),
                                                  n, d_o.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), _lib.stream_ptr()), "td_crown_zonal_dev")
        out, pos, status = d_o.cpu().numpy(), d_p.cpu().numpy(), d_s.cpu().numpy()
    capped = np.flatnonzero(status == 1)
    if capped.size:                                          # the host function decides these crowns alone
        out[capped], pos[capped], status[capped] = _zonal_host(raster, transform, *take_rings(xy, start, capped))
    return out, pos[:, 0].copy(), pos[:, 1:].copy(), status


# ---- crown label rasters (opt-in: ``crown_rasters``) ---------------------------------------------------------------------------
def _u32_values(values, n: int) -> np.ndarray:
    """``values`` as uint32 [n]: integers in [0, 2^32) only."""
    v = np.asarray(values)
    if n == 0 and v.size == 0:
        return np.zeros(0, np.uint32)
    if v.shape != (n,) or v.dtype.kind not in "iu":
        raise ValueError(f"crown_label_raster: values must be {n} unsigned integers below 2^32, got {v.dtype} {v.shape}")
    if n and (int(v.min()) < 0 or int(v.max()) >= 1 << 32):
        raise ValueError("crown_label_raster: values must be unsigned integers below 2^32")
    return np.array(v, dtype=np.uint32)                      # (a copy of its own: writable, C-contiguous)


def _labels_host(labels: np.ndarray, transform, xy: np.ndarray, start: np.ndarray, values: np.ndarray) -> np.ndarray:
    """td_crown_labels over ``labels`` (uint32 [rows, cols], C-contiguous) in place → status int32 [n]."""
    n = start.size - 1
    status = np.empty(n, np.int32)
    _lib.check(_lib.load().td_crown_labels(labels.shape[0], labels.shape[1], _lib.transform6(transform), nonempty(xy).ctypes.data, xy.shape[0],
                                           start.ctypes.data, nonempty(values).ctypes.data, n, labels.ctypes.data, status.ctypes.data), "td_crown_labels")
    return status


def crown_label_raster(rings, values, transform, shape, device: Optional[int] = 0, out=None, packed=None, uploaded=None):
    """Crown outlines drawn into a label raster → (labels uint32 [rows, cols], status int32 [n]):
    ``labels[r, c] = max(labels before, max{values[q] : the centre of pixel (r, c) belongs to ring q})`` (include/treedet.h,
    td_crown_labels; membership is crown_zonal_stats's). The maximum is unsigned and order-free, so the raster is the same bits on
    the host and on the device. ``values``: one unsigned integer below 2^32 per ring (anything else: ValueError); 0 draws nothing.
    ``transform``, ``shape`` = (rows, cols): the grid. ``device``: None — td_crown_labels on numpy arrays; ``out``, a C-contiguous
    uint32 array [rows, cols], is composited over in place. A GPU index — td_crown_labels_dev, a wave per crown, on a tensor that is
    allocated and zeroed unless ``out`` is given: a contiguous CUDA tensor [rows, cols] of 32-bit integers (int32 holds the bits
    where torch.uint32 lacks an op), drawn over where it lies and returned as it is; without ``out`` the labels come back as a
    numpy uint32 array. Crowns the kernel leaves out (status 1: more than ``_lib.ZONAL_RING_CAP`` vertices) are drawn by the host
    function after the download and merged with np.maximum — the same raster, the rule being order-free —, their status the
    host's. Refused crowns (status 2) draw nothing. ``packed`` / ``uploaded`` as for crown_zonal_stats."""
    xy, start = packed if packed is not None else pack_rings(rings)
    n = start.size - 1
    vals = _u32_values(values, n)
    rows, cols = int(shape[0]), int(shape[1])
    if rows < 1 or cols < 1 or rows * cols >= 1 << 31:
        raise ValueError(f"crown_label_raster: a {rows} x {cols} raster: both at least 1 and fewer than 2^31 pixels")
    if device is None:
        if out is None:
            out = np.zeros((rows, cols), np.uint32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.shape == (rows, cols) and out.flags.c_contiguous):
            raise ValueError(f"crown_label_raster: out must be a C-contiguous uint32 array [{rows}, {cols}]")
        return out, _labels_host(out, transform, xy, start, vals)
    given = out is not None
    if given and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (torch.int32, torch.uint32) and tuple(out.shape) == (rows, cols)
                      and out.is_contiguous()):
        raise ValueError(f"crown_label_raster: out must be a contiguous int32 / uint32 CUDA tensor [{rows}, {cols}]")
    dev = out.device if given else torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_l = out if given else torch.zeros((rows, cols), dtype=torch.int32, device=dev)
        if n == 0:
            return (d_l if given else np.zeros((rows, cols), np.uint32)), np.zeros(0, np.int32)
        d_xy, d_start = uploaded if uploaded is not None else upload_rings(xy, start, dev)
        d_v = torch.from_numpy(vals.view(np.int32)).to(dev)
        d_s = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().td_crown_labels_dev(rows, cols, _lib.transform6(transform), d_xy.data_ptr(), xy.shape[0], d_start.data_ptr(),
                                                   d_v.data_ptr(), n, d_l.data_ptr(), d_s.data_ptr(), _lib.stream_ptr()), "td_crown_labels_dev")
        status = d_s.cpu().numpy()
        capped = np.flatnonzero(status == 1)
        if not capped.size:
            return (d_l if given else d_l.cpu().numpy().view(np.uint32)), status
        # the host function draws these crowns alone, into a raster of their own; the maximum of the two is the whole rule
        extra = np.zeros((rows, cols), np.uint32)
        status[capped] = _labels_host(extra, transform, *take_rings(xy, start, capped), np.ascontiguousarray(vals[capped]))
        merged = np.maximum(d_l.cpu().numpy().view(np.uint32), extra)
        if not given:
            return merged, status
        d_l.copy_(torch.from_numpy(merged.view(np.int32)).to(dev).view(d_l.dtype))
        return d_l, status


def crown_priorities(scores, labels=None):
    """Distinct drawing priorities for crowns that may overlap → (priority uint32 [n], table uint32 [n + 1]). The higher score gets
    the higher priority; among equal scores the LOWER index does; the priorities are 1 .. n, so under crown_label_raster's maximum
    a pixel goes to the best crown that holds it. ``table[priority[k]] = labels[k]`` (default k + 1) and ``table[0] = 0`` take a
    raster of composited priorities back to labels (labels_from_priorities). NaN scores are refused."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    n = s.size
    if np.isnan(s).any():
        raise ValueError("crown_priorities: a score is NaN")
    if n >= (1 << 31) - 1:
        raise ValueError("crown_priorities: too many crowns")
    order = np.lexsort((-np.arange(n), s))                  # ascending score; among equal scores descending index
    priority = np.empty(n, np.uint32)
    priority[order] = np.arange(1, n + 1, dtype=np.uint32)
    table = np.zeros(n + 1, np.uint32)
    table[priority] = np.arange(1, n + 1, dtype=np.uint32) if labels is None else _u32_values(labels, n)
    return priority, table


def labels_from_priorities(raster, table: np.ndarray):
    """A raster of composited priorities (crown_label_raster over crown_priorities' values) → the labels, ``table[raster]``. A CUDA
    tensor of 32-bit integers is looked up on the device, through 32-bit indices — no temporary larger than the raster — and comes
    back as a tensor of the same dtype; a numpy array gives a numpy uint32 array."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    if isinstance(raster, torch.Tensor):
        d_t = torch.from_numpy(table.view(np.int32)).to(raster.device)
        idx = raster.view(torch.int32).reshape(-1)          # priorities are at most n < 2^31: the bits are the index
        return torch.index_select(d_t, 0, idx).view(raster.dtype).reshape(raster.shape)
    return table[np.asarray(raster)]
