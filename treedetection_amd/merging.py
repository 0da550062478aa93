"""Seam strips between neighbouring images (reference TreeDetection/merging.py:10-118 ``merge_and_crop_images`` with
helpers.py ``retrieve_neighboring_image_filenames`` 984-1021, ``merge_images`` 1023-1051, ``crop_image`` 1053-1085).

With ``use_overlap`` the reference mosaics every image with its right and its bottom neighbour (rasterio.merge), cuts
a strip ``(tile + 2*buffer) * overlapping_tiles`` pixels wide out of the middle of the mosaic — the seam — writes it to
``<dir>/<merged_path>/`` and appends it to the work list, so crowns cut by an image border are predicted whole once.
Same steps here on :class:`treedetection_amd.geotiff.GeoTiff` (no rasterio): neighbours by origin arithmetic,
mosaic = rasterio.merge's "first" rule on the union extent at the first image's resolution (oracle/merging_ref.py),
centre crop, uncompressed GeoTIFF out; same file names, same ordering of the appended paths.

``device_seams: true`` (default false): a strip needs a band a few tiles wide on either side of the seam, not two whole rasters.
:func:`seam_windows` works the two raster windows out from the transforms alone, ``GeoTiff.decode_to_device(window=...)`` reads and
decodes only the blocks they touch on the GPU, td_seam_first_dev (csrc/seam.hip) applies the "first" rule to the two covers in one
launch, and the strip comes back through pinned memory for the same ``write_geotiff`` call — the same files, byte for byte. Pairs the
device decoders do not take (uncompressed files, other sample types, ...) keep the host path above.
"""
from __future__ import annotations

import os
import warnings
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np

from .config import Config
from .geotiff import GeoTiff, _true_false_setting, device_decode_planar_setting, write_geotiff


def tif_geoinfo(filename) -> Tuple[tuple, Optional[int], int, int]:
    g = GeoTiff(filename)
    return g.transform, g.epsg, g.width, g.height


def retrieve_neighboring_image_filenames(filename, other_filenames, meta_info: Optional[Dict[str, tuple]] = None):
    """(left, right, up, down) neighbours of ``filename``: images whose origin lies exactly one image width / height
    away (eps 1e-3), as the reference computes it — offsets use the OTHER image's pixel size and THIS image's size."""
    transform, _, width, height = tif_geoinfo(filename)
    x, y = transform[2], transform[5]
    left = right = up = down = None
    eps = 1e-3
    for other in other_filenames:
        if other == filename:
            continue
        ot = meta_info[other] if meta_info is not None else tif_geoinfo(other)[0]
        oa, oc, of = ot[0], ot[2], ot[5]
        if abs(oc - (x - width * oa)) < eps and abs(of - y) < eps:
            left = other
        if abs(oc - (x + width * oa)) < eps and abs(of - y) < eps:
            right = other
        if abs(of - (y + height * oa)) < eps and abs(oc - x) < eps:
            up = other
        if abs(of - (y - height * oa)) < eps and abs(oc - x) < eps:
            down = other
    return left, right, up, down


def _fill_value(nodata: float, dt: np.dtype) -> float:
    """The value the mosaic starts from. rasterio.merge checks the nodata value against the range of the output dtype and,
    when it does not fit (GDAL_NODATA -9999 on a uint8 raster), warns and leaves the destination at zero.
    DELIBERATE DEVIATION for that case (read from rasterio's source, rasterio is not installed here to confirm):
    rasterio then still compares the destination with the ORIGINAL out-of-range value (``region == -9999`` on uint8 is False
    everywhere), so nothing is ever copied and its mosaic stays all zero — a reference result nobody can want. This port
    compares against the value the destination really holds (0): both images are copied by the "first" rule. For every
    nodata value that fits the dtype — the reference's own rasters — the two agree (tests/test_merging.py)."""
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        if np.isnan(nodata) or not (info.min <= nodata <= info.max) or float(nodata) != int(nodata):
            warnings.warn(f"nodata value {nodata} is beyond the valid range of {dt}: the mosaic starts from 0 (as rasterio.merge does)")
            return 0.0
    return float(nodata)


def _equals(a: np.ndarray, value: float) -> np.ndarray:
    if np.issubdtype(a.dtype, np.integer):
        return a == a.dtype.type(value)
    if np.isnan(value):
        return np.isnan(a)
    return np.isclose(a, value)


def _mosaic_grid(src1: GeoTiff, src2: GeoTiff):
    """The union mosaic of the two rasters on src1's grid, from the transforms and sizes alone: → (nodata as helpers.merge_images
    picks it — src1's unless it is missing or absurd, then 0.0 —, a, e, left, top, W, H)."""
    if src1.epsg != src2.epsg:
        raise ValueError("CRS of the two images do not match.")
    nodata = getattr(src1, "nodata", None)
    if nodata is None or abs(nodata) > 1e10:
        nodata = 0.0
    a, _, c1, _, e, f1 = src1.transform
    _, _, c2, _, _, f2 = src2.transform
    left, top = min(c1, c2), max(f1, f2)
    right = max(c1 + a * src1.width, c2 + src2.transform[0] * src2.width)
    bottom = min(f1 + e * src1.height, f2 + src2.transform[4] * src2.height)
    W, H = int(round((right - left) / a)), int(round((bottom - top) / e))
    return nodata, a, e, left, top, W, H


def _footprint(src: GeoTiff, a, e, left, top, W, H):
    """Where ``src`` lies in that mosaic, clipped at its right and bottom edge: → (row0, col0, h, w)."""
    col0, row0 = int(round((src.transform[2] - left) / a)), int(round((src.transform[5] - top) / e))
    return row0, col0, min(src.height, H - row0), min(src.width, W - col0)


def _own_nodata(src: GeoTiff, sdt: np.dtype):
    """The source's own nodata value when its pixels have to stay out of the mosaic (a tag that cannot occur in the data masks
    nothing), else None."""
    own = getattr(src, "nodata", None)
    if own is not None:
        fits = not np.issubdtype(sdt, np.integer) or (not np.isnan(own) and np.iinfo(sdt).min <= own <= np.iinfo(sdt).max)
        if fits:
            return own
    return None


def merge_images(src1: GeoTiff, src2: GeoTiff):
    """rasterio.merge.merge([src1, src2], nodata=v), method "first", v = src1's nodata unless it is missing or absurd
    (then 0.0): union extent on src1's grid, filled with v; each image in turn is copied where the mosaic STILL HOLDS v
    AND the image's pixel is not one of ITS OWN nodata pixels (rasterio reads every source masked by the source's
    nodata: ``copyto(dest, new, where=dest_is_nodata & ~new_mask)``). A value rule on the destination side: where the
    first image holds v itself a later overlapping image shows through — for the exactly adjacent neighbours the
    reference merges the footprints never overlap. → (data [bands, rows, cols], transform)."""
    nodata, a, e, left, top, W, H = _mosaic_grid(src1, src2)
    dt = src1.dtype.newbyteorder("=")
    nodata = _fill_value(nodata, dt)
    out = np.full((src1.count, H, W), nodata, dtype=dt)
    for src in (src1, src2):
        row0, col0, h, w = _footprint(src, a, e, left, top, W, H)
        data = src.read()
        bands = min(src.count, out.shape[0])
        view = out[:bands, row0:row0 + h, col0:col0 + w]
        new = data[:bands, :h, :w]
        free = _equals(view, nodata)
        own = _own_nodata(src, new.dtype)
        if own is not None:                      # the source's own nodata pixels stay out of the mosaic
            free &= ~_equals(new, own)
        np.copyto(view, new, where=free, casting="unsafe")
    return out, (a, 0.0, left, 0.0, e, top)


def crop_image(data: np.ndarray, transform, width: int, height: int):
    """Centre crop of ``width`` x ``height`` PIXELS (the reference passes metres here; kept). Raises when the window
    does not fit, which is where the reference's ``dest.write`` fails and the strip is skipped."""
    left, top, width, height, ct = _centre_window(data.shape[2], data.shape[1], transform, width, height)
    return data[:, top:top + height, left:left + width], ct


def _centre_window(img_w: int, img_h: int, transform, width, height):
    """crop_image's arithmetic on the mosaic's size alone: → (left, top, width, height, the window's transform)."""
    left = max(img_w // 2 - int(width) // 2, 0)
    top = max(img_h // 2 - int(height) // 2, 0)
    width, height = int(width), int(height)
    if left + width > img_w or top + height > img_h:
        raise ValueError(f"crop window {width}x{height} at ({left},{top}) exceeds the {img_w}x{img_h} mosaic")
    a, b, c, d, e, f = transform
    return left, top, width, height, (a, b, c + a * left + b * top, d, e, f + d * left + e * top)


def _strip_size(config, horizontal: bool, W: int, H: int):
    """The seam strip the reference cuts out of a W x H mosaic: (tile + 2 * buffer) * overlapping_tiles across the seam, the whole
    mosaic along it → (width, height) as handed to :func:`crop_image`."""
    if horizontal:
        return (config["tile_width"] + 2 * config["buffer"]) * config["overlapping_tiles_width"], H
    return W, (config["tile_height"] + 2 * config["buffer"]) * config["overlapping_tiles_height"]


def device_seams_setting(value=False) -> bool:
    """The ``device_seams`` config key: true / false (default) → whether :func:`merge_and_crop_images` cuts the strips of compressed
    rasters on the GPU (below). Anything else is refused."""
    return _true_false_setting("device_seams", value)


def seam_windows(src1: GeoTiff, src2: GeoTiff, horizontal: bool, config):
    """The geometry of one seam strip from the two transforms and sizes alone — nothing is read: what ``crop_image(*merge_images(src1,
    src2), ...)`` would cut, without the mosaic. → a namespace with ``mosaic`` = (H, W) and ``mosaic_transform`` (merge_images'),
    ``strip`` = (top, left, rows, cols) in the mosaic and its ``transform`` (crop_image's arithmetic; a strip that does not fit raises
    its ValueError, "... exceeds ..."), ``fill`` (:func:`_fill_value`, with its warning), and ``sources``: per raster None when its
    footprint (clipped as merge_images clips it) misses the strip, else (window, (row, col)) — the raster window (r0, c0, h, w) that
    intersects the strip and where its first pixel lies in the strip. Filling the strip with ``fill`` and copying each window in
    turn by merge_images' rule gives the strip's pixels."""
    nodata, a, e, left_x, top_y, W, H = _mosaic_grid(src1, src2)
    left, top, cols, rows, ct = _centre_window(W, H, (a, 0.0, left_x, 0.0, e, top_y), *_strip_size(config, horizontal, W, H))
    fill = _fill_value(nodata, src1.dtype.newbyteorder("="))
    sources = []
    for src in (src1, src2):
        row0, col0, h, w = _footprint(src, a, e, left_x, top_y, W, H)
        r_lo, r_hi = max(row0, top), min(row0 + h, top + rows)
        c_lo, c_hi = max(col0, left), min(col0 + w, left + cols)
        if r_lo >= r_hi or c_lo >= c_hi:
            sources.append(None)
        else:
            sources.append(((r_lo - row0, c_lo - col0, r_hi - r_lo, c_hi - c_lo), (r_lo - top, c_lo - left)))
    return SimpleNamespace(mosaic=(H, W), mosaic_transform=(a, 0.0, left_x, 0.0, e, top_y), strip=(top, left, rows, cols), transform=ct,
                           fill=fill, sources=sources)


_SEAM_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.uint16): 2}      # → TD_SAMPLE_* (_lib.SAMPLE_*)


def _cut_on_device(seams, f, other, horizontal, config, planar):
    """One seam strip cut on the GPU (``device_seams``): the two windows of :func:`seam_windows` decoded block by block
    (``GeoTiff.decode_to_device(window=...)``: only the blocks the strip touches are read and decoded), one td_seam_first_dev launch
    over the two covers (csrc/seam.hip: merge_images' rule per sample), the strip copied into a pinned buffer — all on the current
    stream of the current device, from the calling thread. → (the strip as a [bands, rows, cols] VIEW of those [rows, cols, bands]
    bytes, which write_geotiff transposes back for nothing; its transform; the EPSG code; the buffer's slot, whose ``busy`` the
    caller sets to the future that writes the file), or None when the pair keeps the host path: the two rasters differ in sample
    type, band count or pixel size, the type is not uint8 / uint16 / float32, one of them is not ``device_decodable(float_samples=True,
    planar=...)`` (uncompressed files among them) — or a block turns out corrupt (printed, like the crown stage's height raster).
    ``seams``: the pinned staging buffers, reused from pair to pair (one per raster of a pair for the compressed bytes; four for
    strips, a strip's taken again only after its file is written). What merge_images / crop_image raise is raised here, before
    anything is read."""
    first, second = GeoTiff(f), GeoTiff(other)
    dt = np.dtype(first.dtype.newbyteorder("="))
    if not (first.dtype == second.dtype and dt in _SEAM_DTYPES and first.count == second.count
            and (first.transform[0], first.transform[4]) == (second.transform[0], second.transform[4])
            and first.device_decodable(float_samples=True, planar=planar) and second.device_decodable(float_samples=True, planar=planar)):
        return None
    geo = seam_windows(first, second, horizontal, config)
    import torch
    from . import _lib
    _, _, rows, cols = geo.strip
    nbytes = rows * cols * first.count * dt.itemsize
    slot = seams.slots[seams.turn % len(seams.slots)]
    seams.turn += 1
    if slot.busy is not None:
        slot.busy.result()                                      # the file of the strip that lay here is written
        slot.busy = None
    if slot.buf is None or slot.buf.numel() < nbytes:
        slot.buf = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    sources, checks, covers = [], [], []
    try:
        for src, part, pin in zip((first, second), geo.sources, seams.pins):
            if part is None:
                sources.append(None)
                continue
            window, (at_row, at_col) = part
            cover, check = src.decode_to_device(dev, pinned=pin, planar=planar, window=window)
            wr, wc, h, w = check.window
            own = _own_nodata(src, dt)
            if own is not None and dt.kind == "u":
                own = int(dt.type(own))
            sources.append(_lib.SeamSource(data=cover.data_ptr(), pitch=cover.shape[1], rows=cover.shape[0], row0=at_row - wr, col0=at_col - wc,
                                           r_lo=at_row, c_lo=at_col, r_hi=at_row + h, c_hi=at_col + w, has_own=int(own is not None),
                                           own=float(own if own is not None else 0.0)))
            checks.append(check)
            covers.append(cover)
        strip = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().td_seam_first_dev(strip.data_ptr(), rows, cols, first.count, _SEAM_DTYPES[dt], float(geo.fill), sources[0], sources[1],
                                                 _lib.stream_ptr()), "td_seam_first_dev")
        slot.buf[:nbytes].copy_(strip, non_blocking=True)
    finally:
        torch.cuda.current_stream().synchronize()               # the decodes, the strip and its copy: the staging buffers are free again
    try:
        for check in checks:
            check()
    except ValueError as e:
        print(f"device decode of a seam window failed ({e}): using the host reader")
        return None
    hwc = slot.buf[:nbytes].numpy().view(dt).reshape(rows, cols, first.count)
    return hwc.transpose(2, 0, 1), geo.transform, first.epsg or 0, slot


def merge_and_crop_images(config, images_paths: List[str], height_paths: List[str]) -> None:
    """Appends the seam-strip files of the RGBI images to ``images_paths`` and those of the height rasters to
    ``height_paths`` (both lists are extended in place, like the reference)."""
    Config()._load_into_config(config)
    logger = config["logger"]
    merged_directory = config["merged_path"]

    on_device = device_seams_setting(config.get("device_seams", False))
    planar = device_decode_planar_setting(config.get("device_decode_planar", False))

    def pairs_of(paths, rgbi, meta_info, f):
        """→ [(neighbour, horizontal, the strip's path)] of image ``f``: its right neighbour's strip, then its bottom neighbour's."""
        _, right, _, down = retrieve_neighboring_image_filenames(f, paths, meta_info)
        result_directory = f"{os.path.dirname(f)}/{merged_directory}"
        os.makedirs(result_directory, exist_ok=True)
        stem = os.path.basename(f).replace(".tif", "")
        f_basename, f_name_end = stem.split("_")[0], stem.split("_")[-1]
        fx, fy = meta_info[f][2], meta_info[f][5]
        pairs = []
        for other, horizontal in ((right, True), (down, False)):
            if other is None:
                continue
            ox, oy = meta_info[other][2], meta_info[other][5]
            if rgbi:
                name = f"{f_basename}_{round(fx)}_{round(fy)}_{round(ox)}_{round(oy)}_{f_name_end}.tif"
            else:
                name = f"{f_basename}_{round(fx)}{round(fy)}{round(ox)}{round(oy)}_{f_name_end}.tif"
            pairs.append((other, horizontal, f"{result_directory}/{name}"))
        return pairs

    def host_strip(f, other, horizontal, target):
        first, second = GeoTiff(f), GeoTiff(other)
        merged, mt = merge_images(first, second)
        crop, ct = crop_image(merged, mt, *_strip_size(config, horizontal, merged.shape[2], merged.shape[1]))
        write_geotiff(target, np.ascontiguousarray(crop), ct, first.epsg or 0)

    def logged(work, f, other, target):
        """→ ``target`` once ``work()`` has written it, None (and the reference's error line) when it raised."""
        try:
            work()
            return target
        except Exception as e:
            logger.error(f"Error merging images {f} and {other}: {e}")
            return None

    def crop_single_image(paths, rgbi, meta_info, f):
        names = [logged(lambda: host_strip(f, other, horizontal, target), f, other, target)
                 for other, horizontal, target in pairs_of(paths, rgbi, meta_info, f)]
        return [n for n in names if n is not None]

    def save_cropped_images(paths, rgbi=True):
        meta_info = {f: tif_geoinfo(f)[0] for f in paths}
        with ThreadPoolExecutor(max_workers=min(8, max(1, len(os.sched_getaffinity(0))))) as ex:
            if not on_device:
                results = list(ex.map(lambda f: crop_single_image(paths, rgbi, meta_info, f), list(paths)))
                return [n for sub in results for n in sub]
            # device_seams: this thread alone talks to the GPU, pair after pair on the current stream of the current device; the pool
            # writes the files (and serves the pairs that keep the host path), in the same order of names
            jobs = []
            for f in list(paths):
                for other, horizontal, target in pairs_of(paths, rgbi, meta_info, f):
                    cut = []
                    if logged(lambda: cut.append(_cut_on_device(seams, f, other, horizontal, config, planar)), f, other, target) is None:
                        continue                                # (what merge_images / crop_image would have raised: logged, no strip)
                    if cut[0] is None:
                        jobs.append(ex.submit(logged, lambda f=f, o=other, h=horizontal, t=target: host_strip(f, o, h, t), f, other, target))
                    else:
                        view, ct, epsg, slot = cut[0]
                        slot.busy = ex.submit(logged, lambda v=view, c=ct, g=epsg, t=target: write_geotiff(t, v, c, g), f, other, target)
                        jobs.append(slot.busy)
            return [n for n in (j.result() for j in jobs) if n is not None]

    seams = SimpleNamespace(pins=([None], [None]), slots=[SimpleNamespace(buf=None, busy=None) for _ in range(4)], turn=0) if on_device else None
    try:
        cropped_images = save_cropped_images(images_paths, rgbi=True)
        cropped_heights = save_cropped_images(height_paths, rgbi=False)
        images_paths.extend(cropped_images)
        height_paths.extend(cropped_heights)
    except Exception as e:
        logger.error(f"Error merging and cropping images: {e}")
