"""Seam strips cut on the GPU (``device_seams``): td_seam_first_dev (csrc/seam.hip) alone against the strip rule restated in numpy on
``merging._equals``, its float equality on every edge of numpy.isclose, ``GeoTiff.decode_to_device(window=...)`` against the host
reader's windows, and ``merge_and_crop_images`` with the key on against the key off and the oracle, file by file and byte by byte."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle.merging_ref import seam_strips_ref
from treedetection_amd import _lib
from treedetection_amd import merging as M
from treedetection_amd.geotiff import GeoTiff, write_geotiff

from seam_cases import first_rule, rand_raster, windows

pytestmark = pytest.mark.gpu
GUARD = 4096
SAMPLE = {np.dtype(np.uint8): _lib.SAMPLE_U8, np.dtype(np.uint16): _lib.SAMPLE_U16, np.dtype(np.float32): _lib.SAMPLE_F32}
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------
def _seam_dev(dtype, rows, cols, spp, fill, sources):
    """td_seam_first_dev on numpy sources → (the strip [rows, cols, spp], both guards). A source: None, or a dict of ``buf`` [R, pitch,
    spp], ``at`` = strip coordinates of its pixel (0, 0), ``rect`` = (r_lo, c_lo, r_hi, c_hi), ``own``, ``shift`` (bytes its device copy
    is moved off its allocation's alignment), ``null`` (the struct is passed, its data pointer is null)."""
    dt = np.dtype(dtype)
    nbytes = rows * cols * spp * dt.itemsize
    arena = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    keep, structs = [], []
    for s in sources:
        if s is None:
            structs.append(None)
            continue
        raw = torch.from_numpy(np.ascontiguousarray(s["buf"]).view(np.uint8).reshape(-1))
        d = torch.zeros((raw.numel() + 16,), dtype=torch.uint8, device="cuda")
        d[s["shift"]:s["shift"] + raw.numel()] = raw.cuda()
        keep.append(d)
        own = s["own"]
        structs.append(_lib.SeamSource(data=None if s.get("null") else d.data_ptr() + s["shift"], pitch=s["buf"].shape[1], rows=s["buf"].shape[0],
                                       row0=s["at"][0], col0=s["at"][1], r_lo=s["rect"][0], c_lo=s["rect"][1], r_hi=s["rect"][2], c_hi=s["rect"][3],
                                       has_own=int(own is not None), own=float(0.0 if own is None else own)))
    _lib.check(_lib.load().td_seam_first_dev(arena.data_ptr() + GUARD, rows, cols, spp, SAMPLE[dt], float(fill), structs[0], structs[1],
                                             _lib.stream_ptr()), "td_seam_first_dev")
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    return host[GUARD:GUARD + nbytes].view(dt).reshape(rows, cols, spp), host[:GUARD], host[GUARD + nbytes:]


def _reference(dtype, rows, cols, spp, fill, sources):
    parts = []
    for s in sources:
        if s is None or s.get("null"):
            continue
        r_lo, c_lo, r_hi, c_hi = s["rect"]
        parts.append((s["buf"][r_lo - s["at"][0]:r_hi - s["at"][0], c_lo - s["at"][1]:c_hi - s["at"][1]], (r_lo, c_lo), s["own"]))
    return first_rule(np.empty((rows, cols, spp), dtype=dtype), fill, parts)


FLOAT_POOL = np.array([0.0, -0.0, -9999.0, np.nan, 1.0, 3.0e4, 1.000001, 2.5, 1e-40, -1e-40, np.inf, -np.inf, -9998.9, 7.25], dtype=np.float32)


def _samples(rng, dtype, shape):
    """Values that meet the fill and own values often: small integers; floats from a pool with both zeros, NaN, inf, subnormals."""
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, 9, shape).astype(dtype)
    return FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), shape)]


def _variants(rng, dtype, rows, cols, spp):
    """Four launches per shape → [(fill, [first, second])]: origins negative, zero and positive; pitches beyond the window; a None
    second source and a null data pointer; rectangles that cover part of the strip; sources one sample off their alignment."""
    item = np.dtype(dtype).itemsize
    integer = np.dtype(dtype).kind == "u"
    fills = (0, 7, 0, 7) if integer else (0.0, -9999.0, np.nan, 1.0)
    owns = (3, 3, 0, 7) if integer else (-9999.0, np.nan, 3.0e4, 0.0)
    mid = cols // 2

    def src(at, rect, pitch_extra, own=None, shift=0, null=False):
        r_lo, c_lo, r_hi, c_hi = rect
        R, P = r_hi - at[0] + 1, c_hi - at[1] + pitch_extra       # the buffer reaches one row and pitch_extra pixels beyond the rectangle
        return {"buf": _samples(rng, dtype, (R, P, spp)), "at": at, "rect": rect, "own": own, "shift": shift, "null": null}
    left = max(mid - 1, 0)
    return [
        # the first begins above and left of the strip and fills its left part, the second begins inside it; two columns overlap
        (fills[0], [src((-2, -3), (0, 0, rows, min(mid + 1, cols)), 5), src((0, left), (0, left, rows, cols), 3, own=owns[0])]),
        # no second source; the first lies at the strip's origin and may fill its lower right part only
        (fills[1], [src((0, 0), (rows // 2, cols // 3, rows, cols), 7, own=owns[1]), None]),
        # both cover everything, both one sample off their alignment: the second shows through wherever the first holds fill
        (fills[2], [src((-1, -1), (0, 0, rows, cols), 2, shift=item), src((0, 0), (0, 0, rows, cols), 1, own=owns[2], shift=item)]),
        # a first source without data; the second, off alignment with a pitch that moves every row, fills an inner rectangle
        (fills[3], [src((0, 0), (0, 0, rows, cols), 0, null=True), src((-3, -1), (min(1, rows - 1), min(1, cols - 1), rows, cols), 1, own=owns[3], shift=item)]),
    ]


@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("dtype,spp", [(np.uint8, 1), (np.uint8, 3), (np.uint8, 4), (np.uint16, 2), (np.float32, 1)],
                         ids=["u8x1", "u8x3", "u8x4", "u16x2", "f32x1"])
def test_the_kernel_equals_the_numpy_rule_between_untouched_guards(dtype, spp, rows):
    rng = np.random.default_rng(rows * 10 + spp)
    for cols in (1, 3, 4, 5, 63, 64, 65, 255, 257):
        for v, (fill, sources) in enumerate(_variants(rng, dtype, rows, cols, spp)):
            got, lo, hi = _seam_dev(dtype, rows, cols, spp, fill, sources)
            want = _reference(dtype, rows, cols, spp, fill, sources)
            assert (lo == 0xFF).all() and (hi == 0xFF).all(), (cols, v, "a guard was written")
            assert got.tobytes() == want.tobytes(), (cols, v, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4], got.ravel()[:8], want.ravel()[:8])


def test_bad_arguments_are_refused_before_the_launch():
    lib = _lib.load()
    strip = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    buf = torch.zeros((64,), dtype=torch.uint8, device="cuda")

    def call(src=None, **kw):
        a = {"strip": strip.data_ptr(), "rows": 4, "cols": 4, "spp": 1, "sample": _lib.SAMPLE_U8, "fill": 0.0, **kw}
        s = _lib.SeamSource(**{"data": buf.data_ptr(), "pitch": 4, "rows": 4, "row0": 0, "col0": 0, "r_lo": 0, "c_lo": 0, "r_hi": 4, "c_hi": 4,
                               "has_own": 0, "own": 0.0, **(src or {})})
        return lib.td_seam_first_dev(a["strip"], a["rows"], a["cols"], a["spp"], a["sample"], a["fill"], s, None, _lib.stream_ptr())
    assert call() == 0
    cases = [({"strip": None}, None, "null strip"), ({"rows": 0}, None, "strip of"), ({"spp": 5}, None, "samples per pixel"),
             ({"sample": 3}, None, "sample type"), ({}, {"r_hi": 5}, "leaves the"), ({}, {"c_lo": -1}, "leaves the"),
             ({}, {"row0": 1}, "outside its"), ({}, {"col0": -1}, "outside its"), ({}, {"pitch": 3}, "outside its"), ({}, {"rows": 3}, "outside its"),
             ({"fill": 256.0}, None, "fill"), ({"fill": 0.5}, None, "fill"), ({}, {"has_own": 1, "own": -1.0}, "own nodata"),
             ({"sample": _lib.SAMPLE_F32}, {"data": buf.data_ptr() + 2}, "not aligned"),
             ({"sample": _lib.SAMPLE_U16, "strip": strip.data_ptr() + 1}, None, "not aligned")]
    for kw, src, word in cases:
        assert call(src, **kw) == _lib.ERR_INVALID, (kw, src)
        assert word in lib.td_last_error().decode(), (kw, src, lib.td_last_error())
    torch.cuda.synchronize()


# ---- 2. float equality -----------------------------------------------------------------------------------------------------------------
def _sweep(v):
    """float32 samples around every edge of equals(a, v): v itself, v -+ the float32 threshold moved by -2 .. +2 ulps, both zeros, the
    subnormal range, the infinities, NaN."""
    out = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 1.1754944e-38, 1e-8, -1e-8, 1.0000001e-8, 9.999999e-9, np.inf, -np.inf, np.nan,
           3.4028235e38, -3.4028235e38]
    if not np.isnan(v):
        vf = np.float32(v)
        thr = np.float32(1e-8 + 1e-5 * abs(v))
        for edge in (vf, vf - thr, vf + thr, np.float32(np.float64(vf) - np.float64(thr)), np.float32(np.float64(vf) + np.float64(thr))):
            x = np.float32(edge)
            lo = hi = x
            out.append(x)
            for _ in range(2):
                lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
                out += [lo, hi]
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("v", [0.0, -9999.0, 1.0, 3.0e4, float("nan")], ids=str)
def test_float_equality_is_numpy_isclose_on_every_edge(v):
    """As the fill value: the first source holds the sweep, the second a constant, which shows through exactly where equals(sample, fill).
    As an own nodata value: the sample stays out exactly where equals(sample, own)."""
    s = _sweep(v)
    n = len(s)
    first = {"buf": s.reshape(1, n, 1), "at": (0, 0), "rect": (0, 0, 1, n), "own": None, "shift": 0}
    const = {"buf": np.full((1, n, 1), 123.0, dtype=np.float32), "at": (0, 0), "rect": (0, 0, 1, n), "own": None, "shift": 0}
    for fill, sources in ((v, [first, const]), (5.0, [{**first, "own": v}, None]), (v, [{**first, "own": v}, {**const, "own": 123.0}])):
        got, lo, hi = _seam_dev(np.float32, 1, n, 1, fill, sources)
        want = _reference(np.float32, 1, n, 1, fill, sources)
        with np.errstate(invalid="ignore"):
            host_verdict = M._equals(s, fill if sources[0]["own"] is None else v)
        assert got.tobytes() == want.tobytes(), (fill, [(float(a), float(g), float(w), bool(e)) for a, g, w, e in
                                                        zip(s, got.ravel(), want.ravel(), host_verdict) if g.tobytes() != w.tobytes()])
        assert (lo == 0xFF).all() and (hi == 0xFF).all()


# ---- 3. windowed decode ----------------------------------------------------------------------------------------------------------------
RH, RW = 101, 150
PIN = [None]


def _raster(bands, dtype, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:RH, 0:RW]
    img = np.stack([(xx * (b + 1) + yy * 3 + rng.integers(0, 4, (RH, RW))) for b in range(bands)]).astype(np.int64)
    img[:, 20:50, 30:90] = 7                                    # a flat area: long matches
    if dtype == np.uint8:
        return (img % 256).astype(np.uint8)
    if dtype == np.uint16:
        return ((img * 257) % 65536).astype(np.uint16)
    return (img.astype(np.float32) * np.float32(0.37) - np.float32(31.25)).astype(np.float32)


def _same(a, b):
    """Same shape, sample type and bytes (NaN patterns and signed zeros included)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _write(path, img, **kw):
    try:
        write_geotiff(path, img, T, 25832, **kw)
    except ValueError as e:
        if kw.get("compression") == "zstd" and "libzstd" in str(e):
            pytest.skip(str(e))
        raise


SAMPLES = [(np.uint8, 1), (np.uint8, 2), (np.uint16, 1), (np.uint16, 2), (np.float32, 1), (np.float32, 2), (np.float32, 3)]
LAYOUTS = [({"tile": (32, 32)}, False), ({"tile": (32, 32)}, True), ({"rows_per_strip": 8}, False), ({"rows_per_strip": 8}, True)]
# every sample type and predictor in every layout (tiles / strips, chunky / planar); the codec and the band count rotate so that each
# codec meets each sample type, predictor and layout
DECODE_CASES = [(("lzw", "deflate", "zstd")[(i + j) % 3], SAMPLES[i], 1 + (i + j) % 4, LAYOUTS[j]) for i in range(len(SAMPLES)) for j in range(len(LAYOUTS))]


def _decode_id(case):
    codec, (dtype, predictor), bands, (layout, planar) = case
    return f"{codec}-{np.dtype(dtype).name}-p{predictor}-b{bands}-{'tiles' if 'tile' in layout else 'strips'}-{'planar' if planar else 'chunky'}"


@pytest.mark.parametrize("case", DECODE_CASES, ids=_decode_id)
def test_the_window_cut_from_the_cover_is_the_host_readers_window(tmp_path, case):
    codec, (dtype, predictor), bands, (layout, planar) = case
    img = _raster(bands, dtype, bands)
    path = str(tmp_path / "w.tif")
    _write(path, img, compression=codec, predictor=predictor, planar=planar, **layout)
    g = GeoTiff(path)
    assert g.device_decodable(float_samples=True, planar=planar)
    _, whole = g.decode_to_device("cuda:0", planar=planar, pinned=PIN)
    assert _same(whole().cpu().numpy().transpose(2, 0, 1), img)
    assert not hasattr(whole, "origin") and not hasattr(whole, "window")
    bh, bw = g._bh, g._bw
    for name, (r0, c0, h, w) in windows(RH, RW, bh, bw).items():
        cover, check = g.decode_to_device("cuda:0", planar=planar, pinned=PIN, window=(r0, c0, h, w))
        got = check().cpu().numpy()
        by0, bx0, by1, bx1 = r0 // bh, c0 // bw, (r0 + h - 1) // bh, (c0 + w - 1) // bw
        assert check.origin == (by0 * bh, bx0 * bw) and check.window == (r0 - by0 * bh, c0 - bx0 * bw, h, w), name
        assert got.shape == (min((by1 + 1) * bh, RH) - by0 * bh, min((bx1 + 1) * bw, RW) - bx0 * bw, bands) and got.dtype == img.dtype, name
        wr, wc = check.window[:2]
        want = GeoTiff(path)._window_hwc(r0, c0, h, w)
        assert np.ascontiguousarray(got[wr:wr + h, wc:wc + w]).tobytes() == np.ascontiguousarray(want).tobytes(), name
        # the whole cover is the raster's pixels there, not only the window
        oy, ox = check.origin
        assert _same(got.transpose(2, 0, 1), img[:, oy:oy + got.shape[0], ox:ox + got.shape[1]]), name
        if name == "corner":
            assert check.compressed_bytes < whole.compressed_bytes, (check.compressed_bytes, whole.compressed_bytes)
        if name == "whole":
            assert check.compressed_bytes == whole.compressed_bytes


def test_bands_and_window_together_read_one_plane_of_the_sub_grid(tmp_path):
    img = _raster(4, np.uint8, 4)
    path = str(tmp_path / "p.tif")
    _write(path, img, compression="deflate", planar=True, tile=(32, 32))
    g = GeoTiff(path)
    _, every = g.decode_to_device("cuda:0", planar=True, pinned=PIN, window=(40, 40, 30, 30))
    every()
    cover, check = g.decode_to_device("cuda:0", planar=True, pinned=PIN, window=(40, 40, 30, 30), bands=(3, 0))
    got = check().cpu().numpy()
    assert check.origin == (32, 32) and got.shape == (64, 64, 4) and check.compressed_bytes < every.compressed_bytes
    assert np.array_equal(got[:, :, [0, 3]].transpose(2, 0, 1), img[[0, 3], 32:96, 32:96]) and not got[:, :, 1:3].any()
    with pytest.raises(ValueError, match="window"):
        g.decode_to_device("cuda:0", planar=True, window=(90, 0, 20, 20))


@pytest.mark.parametrize("planar", [False, True], ids=["chunky", "planar"])
def test_a_damaged_block_counts_only_inside_the_window_and_by_its_number_in_the_file(tmp_path, planar):
    """LZW codes beyond the table: the decoder reports the block through its status (tests/test_planar_decode_gpu.py's damage)."""
    img = _raster(3, np.uint8, 9)
    good = str(tmp_path / "good.tif")
    _write(good, img, compression="lzw", planar=planar, tile=(32, 32))
    g = GeoTiff(good)
    g._setup_blocks()
    assert (g._nx, g._ny) == (5, 4) and len(g._offs) == (60 if planar else 20)
    hit = (20 if planar else 0) + 6                             # block (1, 1) — of plane 1 in the band-separate file
    raw = bytearray(open(good, "rb").read())
    raw[g._offs[hit] + 2:g._offs[hit] + 6] = b"\xff\xff\xff\xff"
    bad = str(tmp_path / "bad.tif")
    open(bad, "wb").write(bytes(raw))
    outside, inside = (0, 0, 32, 32), (17, 17, 32, 32)          # block 0; blocks 0, 1, 5, 6
    cover, check = GeoTiff(bad).decode_to_device("cuda:0", planar=planar, pinned=PIN, window=outside)
    assert np.array_equal(check().cpu().numpy().transpose(2, 0, 1), img[:, :32, :32])
    cover, check = GeoTiff(bad).decode_to_device("cuda:0", planar=planar, pinned=PIN, window=inside)
    with pytest.raises(ValueError, match=f"block {hit} "):
        check()
    cover, check = GeoTiff(bad).decode_to_device("cuda:0", planar=planar, pinned=PIN)
    with pytest.raises(ValueError, match=f"block {hit} "):
        check()


# ---- 4. merge_and_crop_images ------------------------------------------------------------------------------------------------------------
class Log:
    def __init__(self):
        self.msgs = []

    def __getattr__(self, name):
        return lambda m: self.msgs.append((name, m))


CFG = {"merged_path": "merged", "tile_width": 6, "tile_height": 5, "buffer": 1, "overlapping_tiles_width": 2, "overlapping_tiles_height": 3}
FORMATS = {"deflate-tiles": ({"compression": "deflate", "tile": (16, 16)}, {np.uint8: 2, np.float32: 3}),
           "lzw-strips": ({"compression": "lzw", "rows_per_strip": 5}, {np.uint8: 1, np.float32: 1})}


def _mosaic(root, sub, bands, dtype, rgbi, fmt, plain=None, tagged=(0, 0)):
    """tests/test_merging.py's 3 x 3 mosaic (64 x 48 px rasters, 10 % zeros; the height grid has a hole in the middle), written in
    ``fmt``; raster ``plain`` uncompressed; the height raster ``tagged`` carries nodata=-9999.0 and such pixels (at (0, 0) it is only
    ever the first raster of a pair, so the mosaic starts from its tag and the oracle, which knows no tags, still agrees)."""
    rng = np.random.default_rng(11)
    gsd, W, H = 0.25, 64, 48
    d = root / sub
    os.makedirs(d)
    kw, predictors = FORMATS[fmt]
    names, rasters = [], []
    for iy in range(3):
        for ix in range(3):
            if (ix, iy) == (1, 1) and not rgbi:
                continue
            arr = rand_raster(rng, bands, H, W, dtype, 0.1)
            nodata = None
            if not rgbi and (ix, iy) == tagged:
                arr[:, rng.random((H, W)) < 0.2] = -9999.0
                nodata = -9999.0
            t = (gsd, 0.0, 500000.0 + ix * W * gsd, 0.0, -gsd, 5400000.0 - iy * H * gsd)
            name = str(d / f"{7000 + iy * 3 + ix}_x.tif")
            if plain == (ix, iy):
                write_geotiff(name, arr, t, 25832, nodata=nodata)
            else:
                write_geotiff(name, arr, t, 25832, nodata=nodata, predictor=predictors[dtype], **kw)
            names.append(name)
            rasters.append((arr, t))
    return names, rasters


def _run(root, names, rgbi, device_seams, monkeypatch):
    """merge_and_crop_images on a copy of the folder → (new paths relative to the copy, {relative path: file bytes}, device cuts, log)."""
    src = os.path.dirname(names[0])
    d = str(root / f"run_{device_seams}")
    shutil.copytree(src, d)
    paths = [os.path.join(d, os.path.basename(n)) for n in names]
    cuts = []
    real = M._cut_on_device

    def counted(*a, **kw):
        out = real(*a, **kw)
        cuts.append(out is not None)
        return out
    monkeypatch.setattr(M, "_cut_on_device", counted)
    cfg = {**CFG, "logger": Log(), "device_seams": device_seams}
    imgs, hts = (list(paths), []) if rgbi else ([], list(paths))
    M.merge_and_crop_images(cfg, imgs, hts)
    monkeypatch.setattr(M, "_cut_on_device", real)
    new = (imgs if rgbi else hts)[len(paths):]
    log = [(level, str(m).replace(d, ".")) for level, m in cfg["logger"].msgs]
    return [os.path.relpath(n, d) for n in new], {os.path.relpath(n, d): open(n, "rb").read() for n in new}, cuts, log, new


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("sub,bands,dtype,rgbi", [("rgb", 4, np.uint8, True), ("ndsm", 1, np.float32, False)], ids=["u8x4", "f32x1"])
def test_device_strips_are_the_host_strips_byte_for_byte_and_the_oracles(tmp_path, monkeypatch, sub, bands, dtype, rgbi, fmt):
    names, rasters = _mosaic(tmp_path, sub, bands, dtype, rgbi, fmt)
    want = seam_strips_ref([os.path.basename(n) for n in names], rasters, CFG, rgbi)
    assert len(want) == (12 if rgbi else 8)
    off, off_files, off_cuts, off_log, _ = _run(tmp_path, names, rgbi, False, monkeypatch)
    on, on_files, on_cuts, on_log, on_paths = _run(tmp_path, names, rgbi, True, monkeypatch)
    assert not off_cuts and on_cuts == [True] * len(want)        # every pair of compressed rasters took the device path
    assert on == off == [os.path.join("merged", w[0]) for w in want]
    assert not off_log and not on_log
    for rel, path, (fn, data, t) in zip(on, on_paths, want):
        assert on_files[rel] == off_files[rel], rel
        g = GeoTiff(path)
        assert g.read().tobytes() == data.tobytes() and g.read().shape == data.shape, fn
        assert np.allclose(g.transform, t, rtol=0, atol=1e-9), fn


def test_a_tagged_second_raster_and_an_uncompressed_one(tmp_path, monkeypatch):
    """The height raster in the middle of the top row carries the nodata tag: it is the SECOND raster of its left neighbour's pair
    (its -9999 pixels stay out of that strip) and the first of two others. One uncompressed RGBI raster in the middle: its four pairs
    keep the host path. Device and host files are identical."""
    names, rasters = _mosaic(tmp_path / "h", "ndsm", 1, np.float32, False, "deflate-tiles", tagged=(1, 0))
    off, off_files, _, off_log, _ = _run(tmp_path / "h", names, False, False, monkeypatch)
    on, on_files, on_cuts, on_log, on_paths = _run(tmp_path / "h", names, False, True, monkeypatch)
    assert on == off and on_files == off_files and on_cuts == [True] * 8 and not off_log and not on_log
    first_pair = GeoTiff(on_paths[0]).read()                      # 7000 | 7001: the right half comes from the tagged raster
    assert (first_pair[:, :, :8] != 0).any() and not (first_pair == -9999.0).any() and (rasters[1][0][:, :, :8] == -9999.0).any()
    names, rasters = _mosaic(tmp_path / "r", "rgb", 4, np.uint8, True, "lzw-strips", plain=(1, 1))
    want = seam_strips_ref([os.path.basename(n) for n in names], rasters, CFG, True)
    off, off_files, _, off_log, _ = _run(tmp_path / "r", names, True, False, monkeypatch)
    on, on_files, on_cuts, on_log, on_paths = _run(tmp_path / "r", names, True, True, monkeypatch)
    assert on == off == [os.path.join("merged", w[0]) for w in want] and on_files == off_files and not off_log and not on_log
    assert len(on_cuts) == 12 and sum(on_cuts) == 8               # (1, 1) is in four pairs
    for path, (fn, data, t) in zip(on_paths, want):
        assert GeoTiff(path).read().tobytes() == data.tobytes(), fn


def test_jpeg_rasters_ignore_the_window_and_give_the_same_strips(tmp_path, monkeypatch):
    """JPEG rasters are device-decodable too: they decode whole (origin (0, 0), the window's place inside is its place in the raster)
    and the strips equal the host path's, whose reader decodes the same blocks to the same bytes."""
    rng = np.random.default_rng(4)
    d = tmp_path / "rgb"
    os.makedirs(d)
    names = []
    for ix in range(2):
        names.append(str(d / f"{7000 + ix}_x.tif"))
        write_geotiff(names[-1], rand_raster(rng, 3, 48, 64, np.uint8, 0.1), (0.25, 0.0, 500000.0 + ix * 16.0, 0.0, -0.25, 5400000.0), 25832,
                      compression="jpeg", tile=(16, 16))
    g = GeoTiff(names[0])
    assert g.device_decodable(float_samples=True)
    cover, check = g.decode_to_device("cuda:0", window=(5, 50, 20, 10))
    assert check.origin == (0, 0) and check.window == (5, 50, 20, 10) and tuple(check().shape) == (48, 64, 3)
    off, off_files, _, off_log, _ = _run(tmp_path, names, True, False, monkeypatch)
    on, on_files, on_cuts, on_log, _ = _run(tmp_path, names, True, True, monkeypatch)
    assert on_cuts == [True] and len(on) == 1 and on == off and on_files == off_files and not off_log and not on_log


def test_a_corrupt_block_in_a_seam_window_is_printed_and_the_pair_takes_the_host_path(tmp_path, monkeypatch, capsys):
    names, rasters = _mosaic(tmp_path, "rgb", 4, np.uint8, True, "lzw-strips")
    g = GeoTiff(names[0])
    g._setup_blocks()
    raw = bytearray(open(names[0], "rb").read())
    raw[g._offs[9] + 2:g._offs[9] + 6] = b"\xff\xff\xff\xff"      # the last strip of the top-left raster: inside both of its seam windows
    open(names[0], "wb").write(bytes(raw))
    off, off_files, _, off_log, _ = _run(tmp_path, names, True, False, monkeypatch)
    capsys.readouterr()
    on, on_files, on_cuts, on_log, _ = _run(tmp_path, names, True, True, monkeypatch)
    text = capsys.readouterr().out
    assert "block 9 " in text and "using the host reader" in text
    assert sum(on_cuts) == len(on_cuts) - 2 and len(on_cuts) == 12     # both pairs of the damaged raster: its right seam spans every strip
    assert on == off and on_files == off_files and [m for _, m in on_log] == [m for _, m in off_log]
