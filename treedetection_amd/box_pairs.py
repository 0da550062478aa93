"""Sparse box-pair producers of the crown stage: the pair tests of postprocessing.py's two box filters on the GPU (crownpairs.hip;
opt-in ``device_filters: true``; the host restatements' arithmetic and results), the candidate pairs within a layer they give
:mod:`cleaning`, and those between two box sets (boxpairs_ab.hip and its host twin) that :mod:`evaluation` starts from. Both kernel
families store through crown_device.sparse_rows and stop at MAX_DEVICE_PAIRS.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import _lib
from .crown_device import decline, sparse_rows

MAX_DEVICE_PAIRS = 1 << 27      # pairs a device path stores (512 MB of int32 indices); beyond it the host function serves
MAX_BOX_SPAN = float(1 << 24)   # layer extent (in its units) up to which the float32 pair kernels serve candidate_pairs


def _boxes_declined(bb: np.ndarray) -> Optional[str]:
    """Why the pair kernels must not see these float32 boxes (they skip disjoint pairs, which is only the reference's answer for
    finite boxes of finite positive area), or None."""
    if not np.isfinite(bb).all():
        return "a box coordinate is not finite"
    with np.errstate(over="ignore", invalid="ignore"):
        area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    if not (np.isfinite(area) & (area > 0)).all():
        return "a box has no finite positive float32 area"
    return None


def _weak_threshold(threshold, dtype):
    """``threshold`` in the type numpy compares an array of ``dtype`` with it in — ``dtype`` itself for a Python number (and for a
    numpy scalar that does not widen it) — or None when the comparison would run in a wider type than the kernels compute in."""
    if np.result_type(dtype, threshold) != dtype:
        return None
    with np.errstate(over="ignore"):
        return dtype(threshold)


# ---- the two box filters with the pair tests on the GPU -------------------------------------------------------------------------
def connected_pairs_device(bb: np.ndarray, ar: np.ndarray, iou_thr: np.float32, area_thr: np.float16, device: int = 0):
    """The de-duplication mask of postprocessing.filter_polygons_by_iou_and_area as sparse rows: (row_start int64 [n + 1], cols
    int32 [row_start[n]]) — the j != i with ``mask[i][j]``, row i in ``cols[row_start[i]:row_start[i + 1]]`` in no particular order
    — or None when there are more than MAX_DEVICE_PAIRS of them. td_crown_pairs_count, a prefix sum, td_crown_pairs_fill. ``bb``:
    float32 [n, 4], n >= 1; ``ar``: float16 [n]. The preconditions are the caller's (:func:`filter_polygons_by_iou_and_area_device`)."""
    import torch
    n = bb.shape[0]
    lib = _lib.load()
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_b = torch.from_numpy(np.ascontiguousarray(bb, dtype=np.float32)).to(dev)
        d_a = torch.from_numpy(np.ascontiguousarray(ar, dtype=np.float16)).to(dev)
        args = (d_b.data_ptr(), d_a.data_ptr(), n, float(np.float32(iou_thr)), int(np.float16(area_thr).view(np.uint16)))
        count = lambda c: _lib.check(lib.td_crown_pairs_count(*args, c.data_ptr(), 0.0, None, None, _lib.stream_ptr()), "td_crown_pairs_count")
        fill = lambda rs, cur, cl: _lib.check(lib.td_crown_pairs_fill(*args, rs.data_ptr(), cur.data_ptr(), cl.data_ptr(), _lib.stream_ptr()), "td_crown_pairs_fill")
        rows = sparse_rows(n, count, fill, MAX_DEVICE_PAIRS, dev)
    return None if rows is None else (rows[0], rows[2])


def greedy_removal(row_start: np.ndarray, cols: np.ndarray, conf: np.ndarray, self_connected: Optional[np.ndarray] = None) -> np.ndarray:
    """td_crown_pairs_greedy: the group loop of postprocessing.filter_polygons_by_iou_and_area over sparse rows → removed bool [n].
    ``conf``: float16 [n] without NaN; ``self_connected``: the mask's diagonal (None = set everywhere). Host code."""
    n = len(conf)
    rs = np.ascontiguousarray(row_start, dtype=np.int64)
    cl = np.ascontiguousarray(cols, dtype=np.int32)
    cf = np.ascontiguousarray(conf, dtype=np.float16)
    sc = None if self_connected is None else np.ascontiguousarray(self_connected, dtype=np.uint8)
    if rs.shape != (n + 1,) or (sc is not None and sc.shape != (n,)) or (n and cl.shape != (int(rs[-1]),)):
        raise ValueError("greedy_removal: row_start needs n + 1 entries, cols row_start[n], self_connected n")
    removed = np.zeros(n, np.uint8)
    _lib.check(_lib.load().td_crown_pairs_greedy(rs.ctypes.data, cl.ctypes.data, cf.ctypes.data, None if sc is None else sc.ctypes.data, n,
                                                 removed.ctypes.data), "td_crown_pairs_greedy")
    return removed.astype(bool)


def filter_polygons_by_iou_and_area_device(bounds, areas, confidences, iou_threshold, area_threshold, device=0) -> Optional[List[int]]:
    """postprocessing.filter_polygons_by_iou_and_area with the N x N mask replaced by td_crown_pairs_count / td_crown_pairs_fill
    (sparse rows of connected pairs, the same float32 / float16 arithmetic) and the group loop by td_crown_pairs_greedy → the same
    kept indices. None (one printed line) = use the host function: an input outside what the kernels were argued for — a non-finite
    coordinate, a box without a finite positive float32 area, a NaN confidence, ``iou_threshold`` < 0, a threshold numpy would
    compare in a wider type — or more than MAX_DEVICE_PAIRS connected pairs."""
    who = "filter_polygons_by_iou_and_area_device"
    n = len(areas)
    if n == 0:
        return []
    bb = np.array([[np.float32(v) for v in b] for b in bounds], dtype=np.float32).reshape(-1, 4)
    conf = np.array(confidences, dtype=np.float16)
    ar = np.array(areas, dtype=np.float16)
    iou_thr, area_thr = _weak_threshold(iou_threshold, np.float32), _weak_threshold(area_threshold, np.float16)
    why = _boxes_declined(bb)
    if why is None and np.isnan(conf).any():
        why = "a confidence is NaN"
    if why is None and (iou_thr is None or area_thr is None):
        why = "a threshold is not compared in float32 / float16"
    if why is None and iou_thr < 0:
        why = f"iou_threshold {iou_threshold} is negative"
    if why is not None:
        return decline(who, why)
    pairs = connected_pairs_device(bb, ar, iou_thr, area_thr, device)
    if pairs is None:
        return decline(who, f"more than {MAX_DEVICE_PAIRS} connected pairs")
    # the mask's diagonal, which the sparse rows leave out: it decides how a row's own confidence ties (td_crown_pairs_greedy)
    box_area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        diagonal = (box_area / (box_area + box_area - box_area) > iou_thr) & (np.abs(ar - ar) / np.maximum(ar, ar) < area_thr)
    removed = greedy_removal(pairs[0], pairs[1], conf, diagonal)
    return [int(i) for i in np.flatnonzero(~removed)]


def containment_device(bounds, threshold, device=0):
    """postprocessing.containment with the pair tests in td_crown_pairs_count → the same triple, or None (one printed line) = use
    the host function: a non-finite coordinate, a box without a finite positive float32 area, ``threshold`` <= 0 or compared in a
    wider type than float32. The ratio returned is 1.0 for every box: the diagonal of the ratio matrix is exactly 1 for a finite
    positive area and no entry exceeds it (float subtraction and multiplication are monotone, so iw * ih <= the inner box's area)."""
    b = np.array(bounds, dtype=np.float32).reshape(-1, 4)
    n = b.shape[0]
    if n == 0:
        return [], [], []
    thr = _weak_threshold(threshold, np.float32)
    why = _boxes_declined(b)
    if why is None and thr is None:
        why = "the threshold is not compared in float32"
    if why is None and thr <= 0:
        why = f"containment_threshold {threshold} is not positive"
    if why is not None:
        return decline("containment_device", why)
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_b = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
        out = torch.empty((2, n), dtype=torch.int32, device=dev)
        _lib.check(lib.td_crown_pairs_count(d_b.data_ptr(), None, n, 0.0, 0, None, float(thr), out[0].data_ptr(), out[1].data_ptr(),
                                            _lib.stream_ptr()), "td_crown_pairs_count")
        num, is_c = out.cpu().numpy()
    return [1.0] * n, [bool(v) for v in is_c], [int(v) for v in num]


# ---- candidate pairs within one layer -------------------------------------------------------------------------------------------
def candidate_pairs_host(boxes) -> np.ndarray:
    """int32 [k, 2], i < j, sorted: every pair of float64 boxes (x1, y1, x2, y2) that overlap with positive area — a sweep over
    the boxes sorted by x1. Boxes with a NaN coordinate pair with nothing. Host numpy."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    n = b.shape[0]
    if n < 2:
        return np.zeros((0, 2), np.int32)
    order = np.argsort(b[:, 0], kind="stable")
    s = b[order]
    ends = np.searchsorted(s[:, 0], s[:, 2], side="left")      # the boxes after position r with x1 < x2[r]
    out = []
    for r in range(n):
        e = int(ends[r])
        if e <= r + 1:
            continue
        c = s[r + 1:e]
        hit = (np.minimum(c[:, 2], s[r, 2]) > np.maximum(c[:, 0], s[r, 0])) & (np.minimum(c[:, 3], s[r, 3]) > np.maximum(c[:, 1], s[r, 1]))
        k = np.flatnonzero(hit)
        if k.size:
            j = order[r + 1 + k]
            i = np.full(k.size, order[r])
            out.append(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1))
    if not out:
        return np.zeros((0, 2), np.int32)
    p = np.concatenate(out)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.int32)


def _outward_f32(b: np.ndarray) -> np.ndarray:
    """float64 boxes → float32 boxes that contain them: the lower corner rounded down, the upper corner rounded up."""
    f = b.astype(np.float32)
    lo, hi = f[:, :2], f[:, 2:]
    lo = np.where(lo.astype(np.float64) > b[:, :2], np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < b[:, 2:], np.nextafter(hi, np.float32(np.inf)), hi)
    return np.ascontiguousarray(np.concatenate([lo, hi], axis=1), dtype=np.float32)


def candidate_pairs(boxes, device: int = 0) -> np.ndarray:
    """int32 [k, 2], i < j, sorted: every pair whose float64 boxes overlap with positive area, possibly a few more — the pair
    kernels of the box filters (:func:`connected_pairs_device`: td_crown_pairs_count / td_crown_pairs_fill) asked for
    ``iou > 0``: the boxes are taken relative to the point one unit below and left of the layer's lower-left corner (so no
    coordinate is below 1: two float32 coordinates that differ then differ by at least 2^-23, and the product of two positive
    overlaps cannot underflow to the 0 that ``iou > 0`` would reject) and rounded OUTWARD to float32, so rounding can only add
    pairs; areas all 1, ``iou_threshold`` 0, ``area_threshold`` 1. :func:`candidate_pairs_host` serves when that path declines: a
    non-finite box, a layer wider than 2^24 units, a box without a finite positive float32 area, more than MAX_DEVICE_PAIRS pairs."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    n = b.shape[0]
    if n < 2:
        return np.zeros((0, 2), np.int32)
    why = None
    if not np.isfinite(b).all():
        why = "a box coordinate is not finite"
    else:
        rel = b - np.tile(b[:, :2].min(axis=0) - 1.0, 2)
        if not (rel.max() <= MAX_BOX_SPAN):
            why = f"the layer is wider than {int(MAX_BOX_SPAN)} units"
        else:
            bb = _outward_f32(rel)
            why = _boxes_declined(bb)
    if why is None:
        rows = connected_pairs_device(bb, np.ones(n, np.float16), np.float32(0.0), np.float16(1.0), device)
        if rows is None:
            why = f"more than {MAX_DEVICE_PAIRS} candidate pairs"
    if why is not None:
        decline("candidate_pairs", why)
        return candidate_pairs_host(b)
    p = _pairs_of_rows(np.diff(rows[0]), rows[1], n)        # every pair comes from both of its rows: the one with i < j stays
    return p[p[:, 0] < p[:, 1]]


# ---- candidate pairs between two box sets -----------------------------------------------------------------------------------
def _boxes(b) -> np.ndarray:
    b = np.ascontiguousarray(b, dtype=np.float64)
    if b.size == 0:
        return np.zeros((0, 4))
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"box_pairs_ab: boxes must be [n, 4] (x1, y1, x2, y2), got shape {b.shape}")
    return b


def _pairs_of_rows(counts: np.ndarray, cols: np.ndarray, n_b: int) -> np.ndarray:
    i = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    key = i * max(n_b, 1) + cols
    order = np.argsort(key, kind="stable")
    return np.stack([i[order], cols[order].astype(np.int64)], axis=1).astype(np.int32)


def _box_pairs_ab_host(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    lib = _lib.load()
    counts = np.zeros(a.shape[0], np.int32)
    _lib.check(lib.td_box_pairs_ab(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], counts.ctypes.data, None, 0), "td_box_pairs_ab")
    total = int(counts.sum(dtype=np.int64))
    cols = np.zeros(max(total, 1), np.int32)
    _lib.check(lib.td_box_pairs_ab(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], counts.ctypes.data, cols.ctypes.data, total),
               "td_box_pairs_ab")
    return _pairs_of_rows(counts, cols[:total], b.shape[0])


def box_pairs_ab(boxes_a, boxes_b, device: Optional[int] = 0) -> np.ndarray:
    """int32 [k, 2], sorted lexicographically: every (i, j) whose float64 boxes ``boxes_a[i]`` and ``boxes_b[j]`` (x1, y1, x2, y2)
    overlap with positive area — the pair rule of include/treedet.h: comparisons only, nothing rounded, a box with a NaN pairs with
    nothing, touching boxes are no pair. ``device``: a GPU index (td_box_pairs_ab_count, a prefix sum, td_box_pairs_ab_fill), or
    None for the host twin td_box_pairs_ab — the same set. The device path leaves more than MAX_DEVICE_PAIRS pairs to the host
    twin; an empty set on either side is no launch."""
    a, b = _boxes(boxes_a), _boxes(boxes_b)
    n_a, n_b = a.shape[0], b.shape[0]
    if n_a == 0 or n_b == 0:
        return np.zeros((0, 2), np.int32)
    if device is None:
        return _box_pairs_ab_host(a, b)
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        args = (d_a.data_ptr(), n_a, d_b.data_ptr(), n_b)
        count = lambda c: _lib.check(lib.td_box_pairs_ab_count(*args, c.data_ptr(), _lib.stream_ptr()), "td_box_pairs_ab_count")
        fill = lambda rs, cur, cl: _lib.check(lib.td_box_pairs_ab_fill(*args, rs.data_ptr(), cur.data_ptr(), cl.data_ptr(), _lib.stream_ptr()), "td_box_pairs_ab_fill")
        rows = sparse_rows(n_a, count, fill, MAX_DEVICE_PAIRS, dev)
    if rows is None:
        decline("box_pairs_ab", f"more than {MAX_DEVICE_PAIRS} candidate pairs")
        return _box_pairs_ab_host(a, b)
    return _pairs_of_rows(rows[1], rows[2], n_b)
