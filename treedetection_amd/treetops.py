"""Treetops in a height raster (reference supplementary/pretraining_generate_voronoi.py:32-74, 294-320: ``gaussian_filter``, then the
local maxima of a ``maximum_filter`` above a height — its Voronoi seeds; scipy on one host thread over the full raster, several times):
``td_treetops_dev``, one launch that smooths, takes the window maximum and compares in LDS, and its host twin ``td_treetops`` (any
radius and window; ``device=None``). The rule is stated once, in csrc/treetops.h and include/treedet.h; the Gaussian table is built
HERE with numpy, exactly as scipy builds it, so no ``exp`` of the C library or the device enters a result: the smoothed raster is
``scipy.ndimage.gaussian_filter``'s (float32 in and out) bit for bit, and with a NaN-free raster the treetops are
``argwhere((s == maximum_filter(s, size=window)) & (s > floor))``. The one departure from the reference: it applies ``maximum_filter``
to a copy with NaN where ``s <= 2.5``, whose result where a NaN enters a window depends on scipy's comparison order; here a NaN in a
window is passed over and a NaN pixel is never a treetop.
A layer below postprocessing (which counts treetops per crown with :func:`crown_treetops`, config ``crown_treetops``): it imports
crown_device, crown_rasters, geotiff and gpkg only.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .crown_device import check_raster_tensor, decline
from .crown_rasters import crown_label_raster, crown_priorities, crown_zonal_stats, labels_from_priorities
from .geotiff import GeoTiff
from .gpkg import point_blob, write_blobs

TREETOP_COLUMNS = ("Height", "Row", "Col", "Crown")


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The normalised 1-D Gaussian as scipy.ndimage builds it (_gaussian_kernel1d, order 0) → float64 [2r + 1], r = int(truncate *
    sigma + 0.5). ``sigma == 0`` gives [1.0]: no smoothing. A negative or non-finite sigma is refused."""
    sigma, truncate = float(sigma), float(truncate)
    if not (np.isfinite(sigma) and sigma >= 0 and np.isfinite(truncate) and truncate >= 0):
        raise ValueError(f"gaussian_weights: sigma {sigma}, truncate {truncate}: both finite and not negative")
    r = int(truncate * sigma + 0.5)
    if r == 0:
        return np.ones(1)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def _is_tensor(raster) -> bool:
    return isinstance(raster, torch.Tensor)


def _run(raster, weights: np.ndarray, window: int, floor: float, device: Optional[int], smoothed: bool, counts: bool, who: str):
    """One call of td_treetops_dev or td_treetops → (marks uint8, smoothed float32 or None, counts int32 or None), each [rows, cols]
    or [rows], where the raster lies: CUDA tensors for a tensor raster or a GPU index, numpy arrays for ``device=None`` with a numpy
    raster. Parameters over a device cap go to the host function (decline) and the results back to where the raster lies."""
    if _is_tensor(raster):
        check_raster_tensor(raster, who)
    elif np.ndim(raster) != 2:
        raise ValueError(f"{who}: a raster is [rows, cols], got shape {np.shape(raster)}")
    weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    window, radius = int(window), (weights.size - 1) // 2
    if weights.size != 2 * radius + 1:
        raise ValueError(f"{who}: a weight table holds 2 r + 1 weights, got {weights.size}")
    rows, cols = (int(v) for v in raster.shape)
    lib = _lib.load()
    on_device = _is_tensor(raster) or device is not None
    host = not on_device
    if on_device and (radius > _lib.TREETOP_RADIUS_CAP or window > _lib.TREETOP_WINDOW_CAP):
        decline(who, f"radius {radius} / window {window} over the kernel's {_lib.TREETOP_RADIUS_CAP} / {_lib.TREETOP_WINDOW_CAP}")
        host = True
    if host:
        r = np.ascontiguousarray(raster.cpu().numpy() if _is_tensor(raster) else raster, dtype=np.float32)
        marks = np.empty((rows, cols), np.uint8)
        sm = np.empty((rows, cols), np.float32) if smoothed else None
        cn = np.empty(rows, np.int32) if counts else None
        _lib.check(lib.td_treetops(r.ctypes.data, rows, cols, weights.ctypes.data, radius, window, float(floor), marks.ctypes.data,
                                   sm.ctypes.data if smoothed else None, cn.ctypes.data if counts else None), "td_treetops")
        if not on_device:
            return marks, sm, cn
        dev = raster.device if _is_tensor(raster) else torch.device("cuda", device)
        return tuple(None if a is None else torch.from_numpy(a).to(dev) for a in (marks, sm, cn))
    dev = raster.device if _is_tensor(raster) else torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_r = raster if _is_tensor(raster) else torch.from_numpy(np.ascontiguousarray(raster, dtype=np.float32)).to(dev)
        d_m = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        d_s = torch.empty((rows, cols), dtype=torch.float32, device=dev) if smoothed else None
        d_c = torch.empty(rows, dtype=torch.int32, device=dev) if counts else None
        _lib.check(lib.td_treetops_dev(d_r.data_ptr(), rows, cols, weights.ctypes.data, radius, window, float(floor), d_m.data_ptr(),
                                       d_s.data_ptr() if smoothed else None, d_c.data_ptr() if counts else None, _lib.stream_ptr()),
                   "td_treetops_dev")
    return d_m, d_s, d_c


def _floor(min_height: float) -> float:
    """``min_height`` as the float32 the rule compares with."""
    return float(np.float32(min_height))


def smooth_height(raster, sigma: float, device: Optional[int] = 0):
    """``scipy.ndimage.gaussian_filter(raster, sigma)`` for a float32 raster (mode reflect, truncate 4), bit for bit → float32
    [rows, cols] where the raster lies: a CUDA tensor for a contiguous float32 CUDA tensor (read in place) or a numpy raster with a
    GPU index ``device``; a numpy array for ``device=None`` (the host twin)."""
    return _run(raster, gaussian_weights(sigma), 1, 0.0, device, True, False, "smooth_height")[1]


def treetop_marks(raster, sigma: float = 0.5, window: int = 7, min_height: float = 3.0, device: Optional[int] = 0, smoothed: bool = False,
                  counts: bool = False):
    """The treetops of ``raster`` as a uint8 raster of 1 / 0 where the raster lies (as :func:`smooth_height`). Pixel (r, c) is a
    treetop iff its smoothed height s exceeds ``min_height`` (rounded to float32) and s >= every non-NaN smoothed height in the
    ``window`` x ``window`` pixels around it (include/treedet.h, td_treetops). With ``smoothed`` / ``counts`` → (marks, smoothed
    float32 [rows, cols] or None, counts int32 [rows] = treetops per row, or None)."""
    out = _run(raster, gaussian_weights(sigma), window, _floor(min_height), device, smoothed, counts, "treetop_marks")
    return out if smoothed or counts else out[0]


def pixel_centres(transform, rows: np.ndarray, cols: np.ndarray) -> np.ndarray:
    """float64 [m, 2]: the centres of pixels (rows, cols) under the affine ``transform`` (a, b, c, d, e, f), as td_crown_zonal places
    them: x = (a (col + 0.5) + b (row + 0.5)) + c, y = (d (col + 0.5) + e (row + 0.5)) + f."""
    a, b, c, d, e, f = (float(v) for v in transform[:6])
    cc, rr = np.asarray(cols, np.float64) + 0.5, np.asarray(rows, np.float64) + 0.5
    return np.stack([(a * cc + b * rr) + c, (d * cc + e * rr) + f], axis=1)


def _list_tops(marks, smoothed):
    """marks, smoothed where they lie → (rows int64 [m], cols int64 [m], height float32 [m]) on the host, row-major."""
    if _is_tensor(marks):
        at = torch.nonzero(marks)                                   # row-major, as argwhere
        return at[:, 0].cpu().numpy(), at[:, 1].cpu().numpy(), smoothed[at[:, 0], at[:, 1]].cpu().numpy()
    rows, cols = np.nonzero(marks)
    return rows.astype(np.int64), cols.astype(np.int64), smoothed[rows, cols]


def find_treetops(raster, transform=None, sigma: float = 0.5, window: int = 7, min_height: float = 3.0,
                  device: Optional[int] = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """The treetops of ``raster`` (rule: :func:`treetop_marks`) → (rows int64 [m], cols int64 [m], height float32 [m], xy float64
    [m, 2] or None) in row-major order, as ``argwhere`` gives it. ``height`` is the SMOOTHED value at the treetop. ``xy`` holds the
    pixel CENTRES under ``transform`` (:func:`pixel_centres`; None without one) — the reference seeds its Voronoi cells at the
    pixel's corner, ``transform * (col, row)``, half a pixel up and left. ``raster`` / ``device`` as for :func:`smooth_height`; on
    the device the list comes from ``torch.nonzero`` over the marks and only the treetops travel to the host."""
    marks, smoothed, _ = treetop_marks(raster, sigma, window, min_height, device, smoothed=True)
    rows, cols, height = _list_tops(marks, smoothed)
    return rows, cols, height, (pixel_centres(transform, rows, cols) if transform is not None else None)


# ---- treetops against crowns (postprocessing, config ``crown_treetops``) ---------------------------------------------------------
def crown_treetops(raster, transform, rings, scores, sigma: float = 0.5, window: int = 7, min_height: float = 3.0,
                   device: Optional[int] = 0) -> Tuple[np.ndarray, dict]:
    """Treetops counted per crown and crowns named per treetop → (per_crown int64 [n], tops). ``per_crown[k]`` = the treetops whose
    pixel centre belongs to ``rings[k]`` under td_crown_zonal's membership rule: crown_zonal_stats over the marks as a 0 / 1 float32
    raster, ``rint(mean * count)`` — sums of 0 / 1 are exact in float64 and the float32 mean is off by at most 2^-24 of itself, so
    the product rounds to the count below 2^23 treetops per crown; a refused crown (status 2) counts 0. ``tops`` = {"rows", "cols"
    (int64 [m]), "height" (float32 [m], smoothed), "xy" (float64 [m, 2], pixel centres), "crown" (int64 [m])}: ``crown`` is the
    1-based index of the crown with the highest score that holds the treetop (among equal scores the lower index; crown_priorities
    composited by crown_label_raster, read at the treetops and taken to labels by labels_from_priorities), or 0. ``device``: a GPU
    index, or None for the host functions throughout — the same results either way."""
    n = len(rings)
    marks, smoothed, _ = treetop_marks(raster, sigma, window, min_height, device, smoothed=True)
    rows, cols, height = _list_tops(marks, smoothed)
    tops = {"rows": rows, "cols": cols, "height": height, "xy": pixel_centres(transform, rows, cols), "crown": np.zeros(rows.size, np.int64)}
    if n == 0:
        return np.zeros(0, np.int64), tops
    shape = tuple(int(v) for v in marks.shape)
    if _is_tensor(marks):
        as_float = marks.to(torch.float32)
        stats, count, _, _ = crown_zonal_stats(as_float, transform, rings, marks.device.index)
        priority, table = crown_priorities(scores)
        with torch.cuda.device(marks.device):
            d_l, _ = crown_label_raster(rings, priority, transform, shape, marks.device.index,
                                        out=torch.zeros(shape, dtype=torch.int32, device=marks.device))
            at_tops = d_l[torch.from_numpy(rows).to(marks.device), torch.from_numpy(cols).to(marks.device)]
            tops["crown"] = labels_from_priorities(at_tops, table).cpu().numpy().view(np.uint32).astype(np.int64)
    else:
        stats, count, _, _ = crown_zonal_stats(marks.astype(np.float32), transform, rings, None)
        priority, table = crown_priorities(scores)
        labels, _ = crown_label_raster(rings, priority, transform, shape, None)
        tops["crown"] = labels_from_priorities(labels[rows, cols], table).astype(np.int64)
    with np.errstate(invalid="ignore"):
        per_crown = np.where(count > 0, np.rint(stats[:, 2].astype(np.float64) * count), 0.0)
    return np.nan_to_num(per_crown, nan=0.0).astype(np.int64), tops


def treetops_path(layer_path: str) -> str:
    """``processed_<name>.gpkg`` → ``processed_<name>_treetops.gpkg``."""
    return os.path.splitext(layer_path)[0] + "_treetops.gpkg"


def write_treetops_layer(path: str, tops: dict, epsg: Optional[int]) -> None:
    """A point layer of treetops (``tops`` as :func:`crown_treetops` gives it; "crown" may be absent): one point per treetop at its
    pixel centre, columns Height (DOUBLE, the smoothed height), Row, Col and Crown (INTEGER)."""
    xy = np.asarray(tops["xy"], np.float64).reshape(-1, 2)
    m = xy.shape[0]
    srs_id = int(epsg) if epsg else 4326
    crown = tops.get("crown")
    columns = {"Height": [float(v) for v in tops["height"]], "Row": [int(v) for v in tops["rows"]], "Col": [int(v) for v in tops["cols"]],
               "Crown": [int(v) for v in (crown if crown is not None else np.zeros(m, np.int64))]}
    extent = (float(xy[:, 0].min()), float(xy[:, 1].min()), float(xy[:, 0].max()), float(xy[:, 1].max())) if m else None
    write_blobs(path, (point_blob(x, y, srs_id) for x, y in xy), columns if m else {}, epsg, extent, geometry_type="POINT")


def treetops_file(height_path: str, out_gpkg: str, sigma: float = 0.5, window: int = 7, min_height: float = 3.0, device: Optional[int] = 0,
                  device_decode: bool = False) -> int:
    """The treetops of the single-band raster at ``height_path`` as a point layer ``out_gpkg`` (:func:`write_treetops_layer`, Crown
    0 throughout; CRS and transform from the raster's header) → how many. ``device_decode``: a raster the device decoders take
    (``GeoTiff.device_decodable(float_samples=True)``) is decoded in HBM and read there; anything else, and every raster without
    it, is read on the host and copied. ``device=None``: the host twin."""
    g = GeoTiff(height_path)
    try:
        if g.count != 1:
            raise ValueError(f"{height_path}: a height raster has one band, this one has {g.count}")
        raster = None
        if device is not None and device_decode and g.device_decodable(float_samples=True):
            try:
                raster = g.decode_to_device(torch.device("cuda", device))[1]().view(g.height, g.width)
            except ValueError as e:
                print(f"device decode of {height_path} failed ({e}): using the host reader")
        if raster is None:
            raster = np.ascontiguousarray(g.read()[0], dtype=np.float32)
        transform, epsg = g.transform, g.epsg
    finally:
        g.close()
    rows, cols, height, xy = find_treetops(raster, transform, sigma, window, min_height, device)
    write_treetops_layer(out_gpkg, {"rows": rows, "cols": cols, "height": height, "xy": xy}, epsg)
    return int(rows.size)
