"""Crown post-processing (reference TreeDetection/postprocessing.py): confidence / area filters, box-IoU de-duplication, per-crown
height and NDVI statistics from the nDSM and RGBI rasters, height / NDVI / border / containment selection, attributes (Area,
TreeHeight, Centroid, Diameter, is_contained, num_contained) and the ``processed_*.gpkg`` layers — the only consumer of the nDSM
side band. This is the top of the crown stage: the device wrappers it calls lie below it, in crown_rasters.py,
box_pairs.py and cleaning.py on crown_device.py, and their names are imported here, where callers have always found them.

What runs where: the raster statistics — in the reference a cupy test of every crown against EVERY pixel — are one launch per raster
(bounding circles; ``crown_statistics: polygon``: the OUTLINES); the N x N box filters and the selection rules are small host numpy
that follows the reference line by line *including* its quirks (marked ``# ref:`` below); opt-in, same files without:
``device_filters: true`` (the filters' pair tests on the GPU), ``clean_crowns: true`` (the layer thinned by outline IoU first),
``crown_rasters: height | image`` (a uint32 label raster written beside the layer, :func:`write_crown_raster`), ``crown_treetops:
true`` (the treetops of the height raster counted per crown and written as a point layer, treetops.py). GDAL's bilinear
decimation of the rasters (``ndvi_scaling_factor`` 0.2 in the example config) is restated from its published algorithm
(:func:`resample_bilinear_gdal`); with ``device_decode: true`` the rasters are decoded in HBM and the same taps applied there, NDVI
included (:func:`resample_on_device`). Not reproduced: fiona's schema handling (:mod:`treedetection_amd.gpkg` writes the layer) and
cupy's float32 reduction order for mean / variance / centroid (accumulated in float64, rounded once). The reference holds no fixture
for this stage: parity is unpinned (oracle/postprocess_ref.py).
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml

from . import _lib
from .box_pairs import MAX_DEVICE_PAIRS, connected_pairs_device, containment_device, filter_polygons_by_iou_and_area_device, greedy_removal  # noqa: F401
from .cleaning import clean_crowns, clean_crowns_setting
from .crown_device import pack_rings, upload_rings
from .crown_rasters import _window, crown_circles, crown_label_raster, crown_priorities, crown_stats, crown_zonal_stats, labels_from_priorities  # noqa: F401
from .geotiff import GeoTiff, device_decode_long_jpeg_setting, device_decode_planar_setting, device_decode_setting, write_geotiff
from .gpkg import polygon_blob, read_layer, write_blobs
from .stitching import simplify_ring
from .treetops import crown_treetops, find_treetops, treetops_path, write_treetops_layer  # noqa: F401

# config.py of the reference defaults none of these four (the stage raises AttributeError without them); its
# example/config.yml sets them and documents 0.2 / 1.0 as the scaling defaults. The NDVI thresholds have no documented
# default: neutral values (filter off) are used when the keys are absent.
DEFAULTS = {"height_scaling_factor": 1.0, "ndvi_scaling_factor": 0.2,
            "ndvi_mean_threshold": -1.0, "ndvi_var_threshold": float("inf")}


def _cfg(config, key):
    if key in config and config[key] is not None:
        return config[key]
    if key in DEFAULTS:
        return DEFAULTS[key]
    raise KeyError(f"config key '{key}' is required by the post-processing stage")


# ---- rasters ---------------------------------------------------------------------------------------------
def _decimation_weights(n_src: int, n_dst: int):
    """Taps of GDAL's convolution resampler for a bilinear (triangle) kernel when shrinking n_src → n_dst pixels
    (gcore/overview.cpp GDALResampleChunk_Convolution: kernel radius 1 stretched by the decimation ratio, weights
    1 - |d| with d in destination-pixel units, normalised over the taps that fall inside the raster)."""
    scale = n_dst / n_src
    # the same routine magnifies: its kernel is stretched only when shrinking (dfXScaleWeight = min(scale, 1)), so for n_dst > n_src
    # the radius stays ONE source pixel — plain bilinear interpolation between pixel centres, taps outside the raster dropped and
    # the rest renormalised (the border rows / columns replicate)
    sw = min(scale, 1.0)
    radius = 1.0 / sw
    rows = []
    for j in range(n_dst):
        centre = (j + 0.5) / scale
        start = max(int(math.floor(centre - radius + 0.5)), 0)
        stop = min(int(centre + radius + 0.5), n_src)
        idx = np.arange(start, stop)
        w = np.maximum(0.0, 1.0 - np.abs(sw * (idx - centre + 0.5)))
        if w.sum() <= 0.0:                       # a tap exactly one radius away on both sides: the nearest source pixel
            idx = np.array([min(max(int(centre), 0), n_src - 1)])
            w = np.ones(1)
        rows.append((idx, w / w.sum()))
    return rows


def resample_bilinear_gdal(arr: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """``src.read(out_shape=(bands, out_h, out_w), resampling=Resampling.bilinear)`` (reference postprocessing.py:781-797):
    the separable triangle filter of GDAL's RasterIO — stretched by the ratio when the out_shape is SMALLER (scaling factor below
    1: decimation), one source pixel wide when it is LARGER (factor above 1: interpolation between pixel centres) — float32
    working type, integer rasters rounded half up and clamped. Same shape = plain copy. GDAL is not available here: restated
    from its published source, unpinned."""
    bands, h, w = arr.shape
    if (out_h, out_w) == (h, w):
        return arr
    if out_h < 1 or out_w < 1:
        raise ValueError(f"cannot resample a {h} x {w} raster to {out_h} x {out_w}")
    work = arr.astype(np.float32)
    tmp = np.empty((bands, h, out_w), np.float32)
    for j, (idx, wgt) in enumerate(_decimation_weights(w, out_w)):
        tmp[:, :, j] = work[:, :, idx] @ wgt.astype(np.float32)
    out = np.empty((bands, out_h, out_w), np.float32)
    for i, (idx, wgt) in enumerate(_decimation_weights(h, out_h)):
        out[:, i, :] = np.tensordot(wgt.astype(np.float32), tmp[:, idx, :], axes=([0], [1]))
    if np.issubdtype(arr.dtype, np.integer):
        info = np.iinfo(arr.dtype)
        return np.clip(np.floor(out + 0.5), info.min, info.max).astype(arr.dtype)
    return out.astype(arr.dtype)


def ndvi_from_rgbi(rgbi: np.ndarray) -> np.ndarray:
    """helpers.ndvi_array_from_rgbi (880-895): bands 0 (red) and 3 (NIR) / 255, (nir - red) / (nir + red + 1e-10)."""
    if rgbi.shape[0] < 4:
        raise ValueError(f"the RGBI raster has {rgbi.shape[0]} bands; NDVI needs the near-infrared band (index 3)")
    red = rgbi[0].astype(np.float64) / 255.0
    nir = rgbi[3].astype(np.float64) / 255.0
    return (nir - red) / (nir + red + 1e-10)


def tap_tables(n_src: int, n_dst: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """:func:`_decimation_weights` of one axis flattened for td_resample_gdal_dev: (start[n_dst], count[n_dst], offset[n_dst]) int32
    and one float32 weight array — output j sums ``src[start[j] + k] * weights[offset[j] + k]`` over ``k < count[j]``. The weights
    are ``wgt.astype(np.float32)``, what :func:`resample_bilinear_gdal` multiplies by; the taps of an output are consecutive source
    indices."""
    rows = _decimation_weights(n_src, n_dst)
    start = np.array([int(idx[0]) for idx, _ in rows], dtype=np.int32)
    count = np.array([len(idx) for idx, _ in rows], dtype=np.int32)
    offset = (np.cumsum(count, dtype=np.int64) - count).astype(np.int32)
    weights = np.concatenate([wgt.astype(np.float32) for _, wgt in rows])
    return start, count, offset, weights


def check_tap_tables(table, n_src: int, n_dst: int, axis: str = "") -> None:
    """Refuses (ValueError) a tap table that td_resample_gdal_dev must not see: wrong lengths or types, ``count < 1``, ``start < 0``,
    ``start + count > n_src`` (a tap outside the source) or ``offset + count`` outside the weight array. Host numpy only."""
    start, count, offset, weights = table
    for name, a in (("start", start), ("count", count), ("offset", offset)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == (n_dst,)):
            raise ValueError(f"{axis} tap table: {name} must be an int32 array of {n_dst} entries")
    if not (isinstance(weights, np.ndarray) and weights.dtype == np.float32 and weights.ndim == 1 and weights.size >= 1):
        raise ValueError(f"{axis} tap table: the weights must be a float32 vector")
    s, c, o = start.astype(np.int64), count.astype(np.int64), offset.astype(np.int64)
    if n_dst < 1 or (c < 1).any() or (s < 0).any() or (s + c > n_src).any():
        raise ValueError(f"{axis} tap table reaches outside the {n_src} source samples (start >= 0, count >= 1, start + count <= {n_src})")
    if (o < 0).any() or (o + c > weights.size).any():
        raise ValueError(f"{axis} tap table reaches outside its {weights.size} weights")


def resample_on_device(tensor: torch.Tensor, out_h: int, out_w: int, bands: Sequence[int], mode: str, tables=None) -> torch.Tensor:
    """:func:`resample_bilinear_gdal` of a raster that lies in HBM (td_resample_gdal_dev, resample.hip: the same taps, float32
    accumulation in ascending tap order). ``tensor``: a contiguous CUDA tensor, uint8 [rows, cols, bands] (what
    GeoTiff.decode_to_device returns) or float32 [rows, cols]; ``bands``: the band indices to compute (at most four). ``mode``:
    "f32" → float32 [len(bands), out_h, out_w]; "u8" → uint8, rounded half up and clamped (the host rule for integer rasters);
    "ndvi" (two bands: red, near-infrared) → float32 [out_h, out_w] = ``ndvi_from_rgbi`` of the two rounded bands, rounded once.
    The same size runs the same kernels with :func:`_decimation_weights`'s identity taps (weights 1, 0). ``tables``: (x table, y
    table) as :func:`tap_tables` returns them, instead of the GDAL taps; they are validated on the host before anything is uploaded."""
    if mode not in _lib.RESAMPLE_MODES:
        raise ValueError(f"resample_on_device: mode must be one of {sorted(_lib.RESAMPLE_MODES)}, got {mode!r}")
    what = "resample_on_device: the raster must be a contiguous CUDA tensor, uint8 [rows, cols, bands] or float32 [rows, cols]"
    if not (isinstance(tensor, torch.Tensor) and tensor.is_contiguous()
            and ((tensor.dtype == torch.uint8 and tensor.dim() == 3) or (tensor.dtype == torch.float32 and tensor.dim() == 2))):
        raise ValueError(what)
    h, w = int(tensor.shape[0]), int(tensor.shape[1])
    c = int(tensor.shape[2]) if tensor.dim() == 3 else 1
    out_h, out_w = int(out_h), int(out_w)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"cannot resample a {h} x {w} raster to {out_h} x {out_w}")
    xt, yt = tables if tables is not None else (tap_tables(w, out_w), tap_tables(h, out_h))
    check_tap_tables(xt, w, out_w, "x")
    check_tap_tables(yt, h, out_h, "y")
    if not tensor.is_cuda:                                  # (after the tables: their validation needs no device)
        raise ValueError(what)
    import ctypes as C
    lib = _lib.load()
    dev = tensor.device
    nb = len(bands)
    band_list = (C.c_int32 * max(nb, 1))(*[int(b) for b in bands])
    with torch.cuda.device(dev):
        d_x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in xt]
        d_y = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in yt]
        tmp = torch.empty((max(nb, 1), h, out_w), dtype=torch.float32, device=dev)
        if mode == "ndvi":
            dst = torch.empty((out_h, out_w), dtype=torch.float32, device=dev)
        else:
            dst = torch.empty((max(nb, 1), out_h, out_w), dtype=torch.float32 if mode == "f32" else torch.uint8, device=dev)
        _lib.check(lib.td_resample_gdal_dev(tensor.data_ptr(), _lib.SAMPLE_U8 if tensor.dtype == torch.uint8 else _lib.SAMPLE_F32, h, w, c,
                                            band_list, nb, *[a.data_ptr() for a in d_x], out_w, xt[3].size,
                                            *[a.data_ptr() for a in d_y], out_h, yt[3].size, tmp.data_ptr(), dst.data_ptr(),
                                            _lib.RESAMPLE_MODES[mode], _lib.stream_ptr()), "td_resample_gdal_dev")
    return dst      # (tmp and the tables go back to torch's allocator on the stream the kernels run on: reuse is ordered after them)


def crown_statistics_setting(value="circle") -> str:
    """The ``crown_statistics`` config key: "circle" (default, also for None: the reference's bounding circles, td_crown_stats) or
    "polygon" (the pixels whose centres lie inside the crown's outline, td_crown_zonal_dev). Anything else is refused."""
    value = "circle" if value is None else value
    if not isinstance(value, str) or value not in ("circle", "polygon"):
        raise ValueError(f"crown_statistics must be 'circle' or 'polygon', got {value!r}")
    return value


def crown_rasters_setting(value=False):
    """The ``crown_rasters`` config key: False (default, also for None: no raster), "height" or "image" (the grid the labels are
    drawn on). Anything else is refused."""
    if value is None or value is False:
        return False
    if not isinstance(value, str) or value not in ("height", "image"):
        raise ValueError(f"crown_rasters must be false, 'height' or 'image', got {value!r}")
    return value


def crown_treetops_setting(config) -> Optional[dict]:
    """The ``crown_treetops`` config key with its three parameters: None for false (the default, also for None), else the keyword
    arguments of treetops.crown_treetops — ``treetop_sigma`` (default 0.5: a finite number, not negative), ``treetop_window`` (7: an
    odd integer, at least 1), ``treetop_min_height`` (3.0: a number, not NaN). Anything else is refused."""
    value = config.get("crown_treetops", False)
    if value is None or value is False:
        return None
    if value is not True:
        raise ValueError(f"crown_treetops must be true or false, got {value!r}")
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
    sigma, window, floor = (config.get(k) if config.get(k) is not None else d
                            for k, d in (("treetop_sigma", 0.5), ("treetop_window", 7), ("treetop_min_height", 3.0)))
    if not number(sigma) or not math.isfinite(sigma) or sigma < 0:
        raise ValueError(f"treetop_sigma must be a finite number, not negative, got {sigma!r}")
    if not isinstance(window, (int, np.integer)) or isinstance(window, bool) or window < 1 or window % 2 == 0:
        raise ValueError(f"treetop_window must be an odd integer, at least 1, got {window!r}")
    if not number(floor) or math.isnan(floor):
        raise ValueError(f"treetop_min_height must be a number, got {floor!r}")
    return {"sigma": float(sigma), "window": int(window), "min_height": float(floor)}


# ---- box filters (host numpy, the reference's dtypes) -------------------------------------------------------
def _box_iou(b: np.ndarray) -> np.ndarray:
    xA = np.maximum(b[:, 0][:, None], b[:, 0])
    yA = np.maximum(b[:, 1][:, None], b[:, 1])
    xB = np.minimum(b[:, 2][:, None], b[:, 2])
    yB = np.minimum(b[:, 3][:, None], b[:, 3])
    inter = np.maximum(0, xB - xA) * np.maximum(0, yB - yA)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area[:, None] + area - inter)


def filter_polygons_by_iou_and_area(bounds, areas, confidences, iou_threshold, area_threshold) -> List[int]:
    """postprocessing.py:349-406 → kept indices. ref: float32 boxes, float16 confidences / areas; ``area_threshold``
    is reused as the relative area-difference limit; removed members still vote in later groups."""
    n = len(areas)
    if n == 0:
        return []
    bb = np.array([[np.float32(v) for v in b] for b in bounds], dtype=np.float32).reshape(-1, 4)
    conf = np.array(confidences, dtype=np.float16)
    ar = np.array(areas, dtype=np.float16)
    iou = _box_iou(bb)
    with np.errstate(divide="ignore", invalid="ignore"):
        area_diff = np.abs(ar[:, None] - ar) / np.maximum(ar[:, None], ar)
    mask = (iou > iou_threshold) & (area_diff < area_threshold)
    removed = np.zeros(n, bool)
    for i in range(n):
        if removed[i]:
            continue
        connected = np.append(np.where(mask[i])[0], i)
        best = connected[int(np.argmax(conf[connected]))]
        for j in connected:
            if j != best:
                removed[j] = True
    return [i for i in range(n) if not removed[i]]


def containment(bounds, threshold):
    """postprocessing.py:408-476 on float32 boxes → (ratio[j], is_contained[j], num_contained[j])."""
    b = np.array(bounds, dtype=np.float32).reshape(-1, 4)
    n = b.shape[0]
    iw = np.maximum(0, np.minimum(b[:, 2][:, None], b[:, 2][None, :]) - np.maximum(b[:, 0][:, None], b[:, 0][None, :]))
    ih = np.maximum(0, np.minimum(b[:, 3][:, None], b[:, 3][None, :]) - np.maximum(b[:, 1][:, None], b[:, 1][None, :]))
    inner = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios = (iw * ih) / inner[None, :]
    is_c = ratios >= threshold
    is_c[np.arange(n), np.arange(n)] = False
    num = is_c.sum(axis=1)
    return ([float(ratios[:, j].max()) for j in range(n)], [bool(is_c[:, j].any()) for j in range(n)], [int(v) for v in num])


def _device_filters_on(config) -> bool:
    """``device_filters`` explicitly true: both box-pair filters take the device path. "auto", the default, and false keep the host
    functions (nothing has decided otherwise: DESIGN.md §7). Anything else is refused."""
    value = config.get("device_filters", "auto")
    value = "auto" if value is None else value
    if not any(value is v for v in (True, False)) and value not in ("auto", "true", "false"):
        raise ValueError(f"device_filters must be true, false or 'auto', got {value!r}")
    return value is True or value == "true"


def _near_border(pb, rb, eps) -> bool:
    """helpers.element_is_near_border; rb = (left, bottom, right, top)."""
    return pb[0] < rb[0] + eps or pb[2] > rb[2] - eps or pb[1] < rb[1] + eps or pb[3] > rb[3] - eps


def _round_ring(ring: np.ndarray) -> np.ndarray:
    """utilities.round_coordinates: round(coord * 1000) / 1000 with Python's round (half to even)."""
    return np.array([[round(float(c) * 1000) / 1000 for c in pt] for pt in ring], dtype=np.float64)


def _height_on_device(hg: GeoTiff, h_scale: float, config, device: int):
    """The height raster decoded in HBM (GeoTiff.decode_to_device → float32 CUDA tensor [rows, cols], which td_crown_stats reads
    where it lies: no inflate on the host, no copy of the array) and, when ``height_scaling_factor`` shrinks it, decimated there
    (:func:`resample_on_device`, mode "f32"); or None when the host reader has to serve it: ``device_decode``
    is not explicitly true / "all" (the default "auto" keeps the host reader for this raster: DESIGN.md §7), the raster is not a single-band native float32 LZW / DEFLATE / ZSTD raster (``device_decodable(float_samples=True)``; band-separate by its tag only with ``device_decode_planar: true``), the
    scaling factor enlarges it (a factor above 1 stays host numpy), or a block turns out corrupt (printed, like the prediction stage)."""
    if not _device_decode_on(config):
        return None
    out_h, out_w = int(hg.height * h_scale), int(hg.width * h_scale)
    if hg.count != 1 or not (1 <= out_h <= hg.height and 1 <= out_w <= hg.width):
        return None
    planar = _planar_on(config)
    if not hg.device_decodable(float_samples=True, planar=planar):
        return None
    try:
        _, check = hg.decode_to_device(torch.device("cuda", device), planar=planar)
        height = check().view(hg.height, hg.width)
    except ValueError as e:
        print(f"device decode of {hg.path} failed ({e}): using the host reader")
        return None
    if (out_h, out_w) == (hg.height, hg.width):             # same shape = the raster itself, as resample_bilinear_gdal returns it
        return height
    return resample_on_device(height, out_h, out_w, [0], "f32")[0]


def _device_decode_on(config) -> bool:
    """``device_decode`` explicitly true / "all": the crown stage's rasters take the device path. "auto", the default, keeps the
    host reader for them (nothing has decided otherwise: DESIGN.md §7). Refuses what the Predictor refuses."""
    value = config.get("device_decode", "auto")
    device_decode_setting("auto" if value is None else value)
    return value in (True, "true", "all")


def _long_jpeg_on(config) -> bool:
    """``device_decode_long_jpeg`` as the Predictor reads it: JPEG rasters with segments too long for one lane take the device path too."""
    return device_decode_long_jpeg_setting(config.get("device_decode_long_jpeg", False))


def _planar_on(config) -> bool:
    """``device_decode_planar`` as the Predictor reads it: band-separate rasters take the device path too."""
    return device_decode_planar_setting(config.get("device_decode_planar", False))


# what the last _ndvi_on_device call copied to the device: {"planes": how many were decoded, "compressed_bytes": their bytes} (tests,
# measurements: a band-separate RGBI raster gives up only bands 0 and 3)
ndvi_decode_stats = {"planes": 0, "compressed_bytes": 0}


def _ndvi_on_device(rg: GeoTiff, n_scale: float, config, device: int):
    """The NDVI raster of the crown statistics computed in HBM: the RGBI raster decoded there (GeoTiff.decode_to_device), bands 0 and
    3 resampled to [int(rows * n_scale), int(cols * n_scale)] and turned into NDVI by one call of td_resample_gdal_dev (mode "ndvi";
    with ``n_scale`` 1 the same kernels run with identity taps) → float32 CUDA tensor for :func:`crown_stats`. None when the host
    reader has to serve it, by the gating of :func:`_height_on_device`: ``device_decode`` not explicitly true / "all", a raster that
    is not uint8 with four bands in a layout the device decoders take (LZW / DEFLATE / ZSTD / JPEG, pixel-interleaved; JPEG blocks without
    restart markers only with ``device_decode_long_jpeg: true``; band-separate LZW / DEFLATE / ZSTD files only with ``device_decode_planar: true``
    — of those only the planes of bands 0 and 3 are read, copied and decoded, the tensor's other channels are 0), or a corrupt block (printed)."""
    if not _device_decode_on(config):
        return None
    out_h, out_w = int(rg.height * n_scale), int(rg.width * n_scale)
    long_jpeg, planar = _long_jpeg_on(config), _planar_on(config)
    if rg.dtype != np.uint8 or rg.count < 4 or out_h < 1 or out_w < 1 or not rg.device_decodable(long_segments=long_jpeg, planar=planar):
        return None
    bands = (0, 3) if rg.planar == 2 else None              # NDVI reads red and infrared: the other planes of a band-separate file stay in the file
    try:
        _, check = rg.decode_to_device(torch.device("cuda", device), long_segments=long_jpeg, planar=planar, bands=bands)
        rgbi = check()
        ndvi_decode_stats.update(planes=len(bands) if bands else rg.count, compressed_bytes=check.compressed_bytes)
    except ValueError as e:
        print(f"device decode of {rg.path} failed ({e}): using the host reader")
        return None
    return resample_on_device(rgbi, out_h, out_w, [0, 3], "ndvi")


# ---- one layer -----------------------------------------------------------------------------------------
def process_layer(rings: List[np.ndarray], scores: Sequence[Optional[float]], config, height_path: str, rgbi_path: str,
                  device: int = 0, keep: Optional[dict] = None) -> List[dict]:
    """process_geojson + process_features (postprocessing.py:722-808, 478-720) for the crowns of one image → the list
    of output features ``{"ring": [m,2], "properties": {...}}`` in the reference's order (duplicates included). ``keep``: a dict
    that receives the height raster as the statistics read it, {"height": array or CUDA tensor, "transform"}, for a caller that
    reads it again (``crown_treetops``)."""
    device_filters = _device_filters_on(config)
    zonal = crown_statistics_setting(config.get("crown_statistics", "circle")) == "polygon"
    conf_thr, iou_thr, area_thr = _cfg(config, "confidence_threshold"), _cfg(config, "iou_threshold"), _cfg(config, "area_threshold")
    h_scale, n_scale = float(_cfg(config, "height_scaling_factor")), float(_cfg(config, "ndvi_scaling_factor"))
    # 1-2: confidence filter, ids, areas of the simplify(2) polygons
    feats = []
    for ring, sc in zip(rings, scores):
        if sc is None or float(sc) < conf_thr:
            continue
        ring = np.asarray(ring, dtype=np.float64)
        simp = simplify_ring(ring, 2.0)
        area = abs(0.5 * float(np.dot(simp[:-1, 0], simp[1:, 1]) - np.dot(simp[1:, 0], simp[:-1, 1])))
        feats.append({"poly_id": str(len(feats)), "ring": ring, "score": sc, "area": area})
    if not feats:
        return []
    id_to_area = {f["poly_id"]: f["area"] for f in feats}
    feats = [f for f in feats if area_thr <= f["area"] <= 1000]
    # rasters, decimated by the scaling factors (postprocessing.py:780-797): transform scaled by src / out size
    hg = GeoTiff(height_path)
    height = _height_on_device(hg, h_scale, config, device)
    if height is None:
        hraw = hg.read()[:1]
        height = resample_bilinear_gdal(hraw, int(hg.height * h_scale), int(hg.width * h_scale))[0].astype(np.float32)
    h_t = (hg.transform[0] * (hg.width / height.shape[1]), hg.transform[1], hg.transform[2],
           hg.transform[3], hg.transform[4] * (hg.height / height.shape[0]), hg.transform[5])
    h_b = hg.bounds                                       # bounds: left, bottom, right, top
    if keep is not None:
        keep.update(height=height, transform=h_t, full_grid=tuple(height.shape) == (hg.height, hg.width))
    rg = GeoTiff(rgbi_path)
    ndvi = _ndvi_on_device(rg, n_scale, config, device)
    if ndvi is None:
        rraw = rg.read()
        rgbi = resample_bilinear_gdal(rraw, int(rg.height * n_scale), int(rg.width * n_scale))
        ndvi = ndvi_from_rgbi(rgbi).astype(np.float32)
    orig_t = rg.transform
    n_t = (orig_t[0] * (rg.width / ndvi.shape[1]), orig_t[1], orig_t[2], orig_t[3], orig_t[4] * (rg.height / ndvi.shape[0]), orig_t[5])
    n_b = rg.bounds
    hg.close()
    rg.close()
    # 3: box-IoU / area de-duplication
    def bounds_of(f):
        r = f["ring"]
        return (r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max())
    dedup_args = ([bounds_of(f) for f in feats], [id_to_area[f["poly_id"]] for f in feats], [f["score"] for f in feats], iou_thr, area_thr)
    kept = filter_polygons_by_iou_and_area_device(*dedup_args, device=device) if device_filters else None
    if kept is None:                                      # the host function: device_filters off, or the device path declined
        kept = filter_polygons_by_iou_and_area(*dedup_args)
    features = [feats[i] for i in kept]
    if not features:
        return []
    # 4: statistics
    if zonal:         # crown_statistics: polygon — the pixels inside each outline, every raster on its own transform, no half radius
        packed = pack_rings([f["ring"] for f in features])
        uploaded = upload_rings(*packed, torch.device("cuda", device))       # one upload for both launches
        hz = crown_zonal_stats(height, h_t, None, device, packed, uploaded)[0]
        nz = crown_zonal_stats(ndvi, n_t, None, device, packed, uploaded)[0]
        heights, mean_ndvi, var_ndvi = hz[:, 1], nz[:, 2], nz[:, 3]
    else:
        circles = crown_circles([f["ring"] for f in features])
        same_grid = all(abs(a - b) < 1e-5 for a, b in zip(h_t[:6], n_t[:6])) and all(abs(a - b) < 1e-3 for a, b in zip(h_b, n_b))
        if same_grid:     # get_metadata_within_polygon: NDVI in half the radius, both on the NDVI transform / bounds
            hs = crown_stats(height, n_t, n_b, circles, 0, 1.0, device, clamp_shape=height.shape)
            ns = crown_stats(ndvi, n_t, n_b, circles, 1, 0.5, device, clamp_shape=height.shape)
        else:
            hs = crown_stats(height, h_t, h_b, circles, 0, 1.0, device)
            ns = crown_stats(ndvi, n_t, n_b, circles, 1, 1.0, device)
        heights, mean_ndvi, var_ndvi = hs[:, 0], ns[:, 2], ns[:, 3]
    centroids = [(np.float32(f["ring"][:, 0].astype(np.float32).astype(np.float64).mean()),
                  np.float32(f["ring"][:, 1].astype(np.float32).astype(np.float64).mean())) for f in features]
    # preselection: image-border / overlap rules, height and NDVI thresholds
    height_thr = _cfg(config, "height_threshold")
    ndvi_mean_thr, ndvi_var_thr = _cfg(config, "ndvi_mean_threshold"), _cfg(config, "ndvi_var_threshold")
    preselected = []
    for i, f in enumerate(features):
        pb = bounds_of(f)
        if config.get("use_overlap", True):
            if _near_border(pb, n_b, 1.0):
                continue
            img_h, img_w = ndvi.shape
            sx, sy = abs(orig_t[0]), abs(orig_t[4])      # ref: the ORIGINAL image's pixel size, while img_h / img_w are
                                                         # the decimated NDVI raster's — kept as in the reference
            v_merged_h = ((config["tile_height"] + 2 * config["buffer"]) * config["overlapping_tiles_height"]) * sy
            h_merged_w = ((config["tile_width"] + 2 * config["buffer"]) * config["overlapping_tiles_width"]) * sx
            if not (img_h == v_merged_h or img_w == h_merged_w):
                right_b, left_b = n_b[2] - h_merged_w / 2.0, n_b[0] + h_merged_w / 2.0
                top_b, bottom_b = n_b[3] - v_merged_h / 2.0, n_b[1] + v_merged_h / 2.0
                if top_b < pb[1] or bottom_b > pb[3] or left_b > pb[2] or right_b < pb[0]:
                    continue
        if heights[i] < height_thr and heights[i] > -1.0:
            continue
        if (mean_ndvi[i] < ndvi_mean_thr or var_ndvi[i] > ndvi_var_thr) and mean_ndvi[i] > -1.0:
            continue
        preselected.append(f)
    # containment over ALL features of step 3
    contain_args = ([bounds_of(f) for f in features], _cfg(config, "containment_threshold"))
    contained = containment_device(*contain_args, device=device) if device_filters else None
    ratios, is_cont, num_cont = contained if contained is not None else containment(*contain_args)
    info = {f["poly_id"]: {"is_contained": is_cont[j], "num_contained": num_cont[j], "containment_ratio": ratios[j]}
            for j, f in enumerate(features)}
    index_of = {f["poly_id"]: j for j, f in enumerate(features)}
    selected = []
    for i, f in enumerate(preselected):
        pid = f["poly_id"]
        cd = info.get(pid, {"is_contained": False, "num_contained": 0})
        if cd["num_contained"] >= 3:
            continue
        elif cd["num_contained"] == 2:
            # ref: nothing is appended on this branch — a crown containing exactly two others is dropped
            continue
        elif cd["num_contained"] == 1:
            # ref: "the other polygon" is the FIRST contained polygon of the whole list, not the one this crown contains
            other_id = [g["poly_id"] for g in features if info[g["poly_id"]]["is_contained"]][0]
            other = features[index_of[other_id]]
            if abs(mean_ndvi[index_of[pid]] - mean_ndvi[index_of[other_id]]) > 0.05:
                if var_ndvi[i] < var_ndvi[index_of[other_id]]:      # ref: var_ndvi[i] — position in the PREselected list
                    selected.append(f)
                else:
                    selected.append(other)
            elif id_to_area.get(pid, 0) > 0:                         # ref: the other area is looked up with an int key → 0
                selected.append(f)
        else:
            selected.append(f)
    out = []
    for f in selected:
        pid = f["poly_id"]
        j = index_of[pid]
        area = id_to_area.get(pid)
        cd = info.get(pid, {"is_contained": False, "num_contained": -1})
        props = {"Confidence_score": float(f["score"]), "poly_id": pid, "Area": float(area), "TreeHeight": float(heights[j]),
                 "Centroid": json.dumps({"x": float(centroids[j][0]), "y": float(centroids[j][1])}),
                 "Diameter": float(2 * (area / np.pi) ** 0.5), "is_contained": str(cd["is_contained"]),
                 "num_contained": int(cd["num_contained"])}
        out.append({"ring": _round_ring(f["ring"]), "properties": props})
    return out


COLUMNS = ("Confidence_score", "poly_id", "Area", "TreeHeight", "Centroid", "Diameter", "is_contained", "num_contained")


def process_single_file(file_path, processed_file_path, height_data_path, rgbi_data_path, device_id=0, config=None):
    """postprocessing.py:876-943: one stitched layer → ``processed_<name>.gpkg``; returns ``file_path`` or None on error
    (printed, like the reference)."""
    thin = clean_crowns_setting((config or {}).get("clean_crowns", False))      # (a bad value is refused, not printed)
    crown_statistics_setting((config or {}).get("crown_statistics", "circle"))  # (likewise)
    rasters = crown_rasters_setting((config or {}).get("crown_rasters", False)) # (likewise)
    tops_args = crown_treetops_setting(config or {})                             # (likewise)
    tops, kept_raster = None, {}
    try:
        device = int(str(device_id).replace("cuda:", "") or 0) if str(device_id) != "cpu" else 0
        layer = read_layer(file_path)
        scores = layer.columns.get("Confidence_score", [None] * len(layer))
        layer_rings = layer.rings()
        if thin:        # ``clean_crowns: true``: the layer is thinned by polygon IoU first, rings and scores together (host functions)
            kept = clean_crowns(layer_rings, scores, iou_threshold=0.7, confidence=0, area_threshold=0, device=None)
            layer_rings, scores = [layer_rings[i] for i in kept], [scores[i] for i in kept]
        feats = process_layer(layer_rings, scores, config, height_data_path, rgbi_data_path, device, **({"keep": kept_raster} if tops_args else {}))
        rings = [f["ring"] for f in feats]
        cols = {c: [f["properties"][c] for f in feats] for c in COLUMNS}
        if tops_args:   # ``crown_treetops``: a failure here is printed and costs the column and the point layer, not the layer
            try:
                per_crown, tops = crown_treetops(*_treetop_raster(height_data_path, kept_raster, config, device), rings,
                                                 cols["Confidence_score"], device=device, **tops_args)
                cols["Treetops"] = [int(v) for v in per_crown]
            except Exception as e:
                print(f"Error finding the treetops of {file_path}: {e}")
        if rings:
            xy = np.concatenate(rings)
            extent = (float(xy[:, 0].min()), float(xy[:, 1].min()), float(xy[:, 0].max()), float(xy[:, 1].max()))
        else:
            extent, cols = None, {}
        write_blobs(processed_file_path, (polygon_blob(r, layer.srs_id) for r in rings), cols, layer.srs_id, extent)
    except Exception as e:
        print(f"Error postprocessing file {file_path}: {e}")
        return None
    if tops is not None:
        try:
            write_treetops_layer(treetops_path(processed_file_path), tops, layer.srs_id)
        except Exception as e:
            print(f"Error writing the treetops of {file_path}: {e}")
    if rasters:         # ``crown_rasters``: the layer is written; a failure here is printed and does not lose it
        try:
            write_crown_raster(crown_raster_path(processed_file_path), rings, cols.get("Confidence_score", []),
                               height_data_path if rasters == "height" else rgbi_data_path, device, layer.srs_id)
        except Exception as e:
            print(f"Error writing the crown raster of {file_path}: {e}")
    return file_path


def _treetop_raster(height_path: str, kept: dict, config, device: int):
    """The height raster on its FULL grid for ``crown_treetops`` → (raster, transform): what process_layer's statistics read (``kept``,
    an array or a CUDA tensor) when ``height_scaling_factor`` left the grid alone, else the file read once more at scale 1, in HBM
    when :func:`_height_on_device` takes it."""
    if kept.get("full_grid"):
        return kept["height"], kept["transform"]
    hg = GeoTiff(height_path)
    try:
        height = _height_on_device(hg, 1.0, config, device)
        if height is None:
            height = np.ascontiguousarray(hg.read()[0], dtype=np.float32)
        return height, hg.transform
    finally:
        hg.close()


def crown_raster_path(layer_path: str) -> str:
    """``processed_<name>.gpkg`` → ``processed_<name>_crowns.tif``."""
    return os.path.splitext(layer_path)[0] + "_crowns.tif"


def write_crown_raster(path: str, rings, scores, grid_path: str, device: int = 0, fallback_epsg: Optional[int] = None) -> None:
    """The label raster of one processed layer: single-band uint32 on the FULL grid of the raster at ``grid_path`` (size, transform
    and EPSG from its header), label k + 1 for ``rings[k]``, 0 = no crown (GDAL_NODATA 0), tiled, LZW. Where crowns overlap, the
    higher score wins and among equal scores the lower index (crown_priorities): the priorities are composited on the GPU
    (crown_label_raster) and taken back to labels there (labels_from_priorities)."""
    g = GeoTiff(grid_path)
    rows, cols, t, epsg = g.height, g.width, g.transform, g.epsg
    g.close()
    if t[1] != 0.0 or t[3] != 0.0:
        raise ValueError(f"{grid_path}: a rotated grid cannot be written as a crown raster")
    priority, table = crown_priorities(scores)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_l = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
        d_l, _ = crown_label_raster(rings, priority, t, (rows, cols), device, out=d_l)
        labels = labels_from_priorities(d_l, table).cpu().numpy().view(np.uint32)
    tmp = path + ".part"
    write_geotiff(tmp, labels, t, int(epsg if epsg is not None else fallback_epsg), tile=(256, 256), compression="lzw", nodata=0)
    os.replace(tmp, path)


# ---- resume file (postprocessing.py:827-874) -----------------------------------------------------------------
_PARAM_KEYS = ("tile_width", "tile_height", "buffer", "confidence_threshold", "containment_threshold", "height_threshold",
               "ndvi_mean_threshold", "ndvi_var_threshold", "iou_threshold", "confidence_threshold_stitching", "area_threshold")


def load_recovery_data_with_params(directory, config, logger=None):
    recovery_file = os.path.join(directory, "recovery.yaml")
    processed = set()
    params = {k: (_cfg(config, k) if k in DEFAULTS else config.get(k)) for k in _PARAM_KEYS}
    params = {k: (v if not (isinstance(v, float) and math.isinf(v)) else str(v)) for k, v in params.items()}
    if crown_statistics_setting(config.get("crown_statistics", "circle")) == "polygon":      # (only then: "circle" files stay valid)
        params["crown_statistics"] = "polygon"
    if crown_treetops_setting(config):                    # (likewise: layers written without the column are not taken for done)
        params["crown_treetops"] = crown_treetops_setting(config)
    if os.path.exists(recovery_file):
        try:
            with open(recovery_file) as f:
                data = yaml.safe_load(f)
            if data.get("parameters") == params:
                processed = set(data.get("processed_files", []))
                if logger:
                    logger.info(f"Loaded {len(processed)} previously processed files from recovery.")
            elif logger:
                logger.info("Parameter mismatch with recovery file. Resetting processed files.")
        except Exception as e:
            if logger:
                logger.warning(f"Failed to load recovery file: {e}")
    return params, processed


def save_recovery_data_with_params(directory, params, processed_files, logger=None):
    try:
        with open(os.path.join(directory, "recovery.yaml"), "w") as f:
            yaml.safe_dump({"parameters": params, "processed_files": sorted(p for p in processed_files if p)}, f, sort_keys=False)
        if logger:
            logger.info(f"Saved recovery file with {len(processed_files)} entries.")
    except Exception as e:
        if logger:
            logger.warning(f"Failed to save recovery file: {e}")


def process_files_in_directory(directory, height_directory, image_directory, parallel=True, filename_pattern=None, config=None):
    """postprocessing.py:945-1076: every stitched ``*.gpkg`` of ``directory`` that is not ``processed_*`` and not in the
    resume file → ``processed_<name>.gpkg``, with the image / height rasters found by the identifier regexes (plain
    names first, then the merged-strip patterns, searched recursively)."""
    logger = config.get("logger")
    params, processed = load_recovery_data_with_params(directory, config, logger)
    files = sorted(f for f in os.listdir(directory) if f.endswith(".gpkg") and not f.startswith("processed_"))
    files = [f for f in files if os.path.join(directory, f) not in processed]
    image_pattern, height_pattern = filename_pattern or (None, None)
    image_pattern = re.compile(image_pattern or "(\\d+)\\.tif")
    height_pattern = re.compile(height_pattern or "(\\d+)\\.tif")
    image_merged = re.compile(config.get("image_merged_regex", "FDOP20_(\\d+)_(\\d+)_(\\d+)_(\\d+)_(\\d+)\\.tif"))
    height_merged = re.compile(config.get("height_data_merged_regex", "FDOP20_(\\d+)_(\\d+)\\.tif"))

    def find(base_name, name_pattern, search_pattern, where):
        m = name_pattern.match(base_name + ".tif")
        if not m:
            return None
        want = "".join(m.groups())
        for root, _, names in os.walk(where):
            for n in sorted(names):
                sm = search_pattern.match(n)
                if sm and "".join(sm.groups()[:len(m.groups())]) == want:
                    return os.path.join(root, n)
        return None

    device = config.get("device", "0")
    for filename in files:
        base = os.path.splitext(filename)[0]
        hpath = find(base, image_pattern, height_pattern, height_directory)
        ipath = find(base, image_pattern, image_pattern, image_directory)
        if hpath is None or ipath is None:
            hpath = find(base, image_merged, height_merged, height_directory)
            ipath = find(base, image_merged, image_merged, image_directory)
        if hpath and ipath:
            res = process_single_file(os.path.join(directory, filename), os.path.join(directory, f"processed_{filename}"),
                                      hpath, ipath, device_id=device, config=config)
            if res is not None:
                processed.add(res)
        elif logger:
            logger.warning(f"Height data file not found for: {filename}, searched pattern for base name: {base}")
    save_recovery_data_with_params(directory, params, processed, logger)
