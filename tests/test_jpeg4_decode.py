"""Four-component JPEG (mode 4 of jpeg_core.h: every component sampled 1x1, samples stored as they decode) — what a four-band RGBI
JPEG-in-TIFF raster holds: td_jpeg_decode against Pillow's libjpeg byte for byte, the block reader on libtiff's and the writer's files,
the host plan, and what both refuse.

Polarity. libjpeg hands out the four components as the stream stores them (JCS_CMYK, no transform), and so do libtiff and
td_jpeg_decode. Pillow's JPEG plugin alone reads and writes mode ``CMYK`` in Adobe's inverted polarity (raw mode ``CMYK;I``): its
decode of a stream is 255 minus the stored bytes, for every stream, with or without an Adobe segment. ``pillow()`` therefore returns
both: the plugin's own CMYK decode, and the same libjpeg decode unpacked with raw mode ``CMYK`` (the stored bytes). td_jpeg_decode must
equal the stored bytes, and 255 minus it must equal the plugin's decode — byte equality with Pillow's CMYK decode, the inversion named."""
import io
import struct

import numpy as np
import pytest
from PIL import Image, ImageFile

from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, _jpeg_split, write_geotiff

T = (0.5, 0, 100, 0, -0.5, 200)


def decode(stream: bytes):
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8)
    out = np.zeros(1 << 20, dtype=np.uint8)
    shape = np.zeros(3, dtype=np.int32)
    n = lib.td_jpeg_decode(src.ctypes.data, src.size, out.ctypes.data, out.size, shape.ctypes.data)
    if n < 0:
        return n
    h, w, c = (int(v) for v in shape)
    assert n == h * w * c
    return out[:n].reshape(h, w, c)


def encode(img: np.ndarray, **kw) -> bytes:
    """Pillow's CMYK encoder: four components with ids C M Y K, an Adobe APP14 segment of transform 0, 1x1 sampling unless told."""
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        buf = io.BytesIO()
        kw.setdefault("subsampling", 0)
        Image.fromarray(img, "CMYK").save(buf, "JPEG", **kw)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def pillow(stream: bytes):
    """→ (Pillow's CMYK decode, the same decode without the plugin's inversion: the bytes as stored)."""
    with Image.open(io.BytesIO(stream)) as im:
        assert im.format == "JPEG" and im.mode == "CMYK"
        plugin = np.asarray(im).copy()
    with Image.open(io.BytesIO(stream)) as im:
        im.tile = [(t[0], t[1], t[2], ("CMYK",) + tuple(t[3][1:])) for t in im.tile]
        stored = np.asarray(im).copy()
    assert np.array_equal(plugin, 255 - stored)
    return plugin, stored


def image(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 + 0.3 * c) for c in range(4)], axis=-1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def drop_segment(stream: bytes, marker: int) -> bytes:
    """The stream without its segments of this marker (before SOS)."""
    out, pos = [stream[:2]], 2
    while stream[pos + 1] != 0xDA:
        n = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        if stream[pos + 1] != marker:
            out.append(stream[pos:pos + 2 + n])
        pos += 2 + n
    return b"".join(out) + stream[pos:]


def assert_same(stream: bytes):
    plugin, stored = pillow(stream)
    got = decode(stream)
    assert not isinstance(got, int), f"td_jpeg_decode returned {got}: {_lib.load().td_last_error()}"
    assert got.shape == stored.shape and np.array_equal(got, stored), (got.shape, stored.shape, int((got != stored).sum()))
    assert np.array_equal(255 - got, plugin)


def assert_same_in_every_layout(stream: bytes):
    """With its Adobe segment (transform 0), without it, and as tables + abbreviated stream (libtiff's layout, no Adobe segment)."""
    assert b"Adobe" in stream[:64]
    assert_same(stream)
    bare = drop_segment(stream, 0xEE)
    assert b"Adobe" not in bare and len(bare) == len(stream) - 16
    assert_same(bare)
    tables, block = _jpeg_split(stream)
    assert b"Adobe" not in block and b"\xff\xdb" not in block[:block.index(b"\xff\xda")]
    assert decode(block) == _lib.ERR_UNSUPPORTED                # no tables of its own
    assert_same(tables[:-2] + block[2:])
    assert np.array_equal(decode(bare), decode(stream)) and np.array_equal(decode(tables[:-2] + block[2:]), decode(stream))


SIZES = [(1, 1), (8, 8), (13, 17), (40, 56)]


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("quality", [30, 90, 100])
@pytest.mark.parametrize("size", SIZES)
def test_matches_pillow(size, quality, kind):
    assert_same_in_every_layout(encode(image(*size, kind, seed=quality), quality=quality))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("opts", [{"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3},
                                  {"restart_marker_blocks": 3, "optimize": True}])
@pytest.mark.parametrize("size", SIZES)
def test_optimized_tables_and_restart_intervals(size, opts, kind):
    stream = encode(image(*size, kind, seed=3), quality=90, **opts)
    mcus = -(-size[0] // 8) * -(-size[1] // 8)
    if "restart_marker_blocks" in opts and mcus > opts["restart_marker_blocks"]:
        assert b"\xff\xdd" in stream and b"\xff\xd0" in stream[stream.index(b"\xff\xda"):]
    assert_same_in_every_layout(stream)


def strips_of(g: GeoTiff):
    """Every strip of a four-band raster as the complete stream the host reader builds, and the rows it must hold."""
    g._setup_blocks()
    for by in range(g._ny):
        raw = bytes(g._mm[g._offs[by]:g._offs[by] + g._counts[by]])
        yield by, g._block_rows(by), g._jpeg_tables[2:-2].join([b"\xff\xd8", raw[2:]])


@pytest.mark.parametrize("rows", [96, 107])
@pytest.mark.parametrize("mode", ["RGBA", "CMYK", "RGBX"])
def test_libtiff_written_files(tmp_path, mode, rows):
    """Pillow's TIFF writer through libtiff: RGB + associated alpha, separated, and RGB + one unspecified extra sample (the GDAL layout
    of RGBI, which Pillow itself opens as three bands). 107 rows: a short last strip."""
    a = image(rows, 128, "smooth", seed=9)
    path = str(tmp_path / f"{mode}.tif")
    Image.fromarray(a, mode).save(path, compression="jpeg", quality=85, tiffinfo={278: 32})          # strips of 32 rows
    g = GeoTiff(path)
    assert g.compression == 7 and g.count == 4 and g.planar == 1
    assert int(g.tags[262][0]) == (5 if mode == "CMYK" else 2) and list(g.tags.get(338, [])) == {"RGBA": [2], "CMYK": [], "RGBX": [0]}[mode]
    got = g.read()
    assert got.shape == (4, rows, 128) and hasattr(g, "_jpeg_tables") and g._flat is None       # block by block, not the whole image
    assert g._ny > 1 and (rows == 96 or g._block_rows(g._ny - 1) < g._bh)
    ref = np.empty((rows, 128, 4), np.uint8)
    for by, nrows, stream in strips_of(g):
        plugin, stored = pillow(stream)
        ref[by * g._bh:by * g._bh + nrows] = stored[:nrows]
        assert_same(stream)                                    # td_jpeg_decode on libtiff's blocks (component ids 0 - 3, no Adobe)
    assert np.array_equal(got, ref.transpose(2, 0, 1))
    assert int(np.abs(got.astype(int) - a.transpose(2, 0, 1)).max()) <= 40                      # the bands as written, not inverted
    if mode != "RGBX":
        with Image.open(path) as im:
            assert im.mode == mode and np.array_equal(np.asarray(im).transpose(2, 0, 1), got)
    else:
        with Image.open(path) as im:
            assert im.mode == "RGB"                             # Pillow drops the fourth band: the whole-image fallback cannot serve it
    for r0, c0, h, w in ((0, 0, rows, 128), (5, 3, 40, 70), (rows - 9, 100, 9, 28), (15, 0, 2, 128)):
        assert np.array_equal(g._window_hwc(r0, c0, h, w), ref[r0:r0 + h, c0:c0 + w])
    assert g.device_decodable() is True
    info, segs, sets, ncoef = g._jpeg_plan()
    assert (info[:, 0] == 0).all() and (info[:, 2] == 4).all() and (info[:, 3] == 0).all() and len(sets) == 1
    g.close()


LAYOUTS = [(150, 200, dict(tile=(64, 64))), (70, 100, dict(rows_per_strip=16)), (150, 200, dict(tile=(64, 64), jpeg_tables=True, jpeg_restart=1))]


@pytest.mark.parametrize("h,w,layout", LAYOUTS)
def test_the_writers_four_band_rasters_round_trip(tmp_path, h, w, layout):
    data = image(h, w, "smooth", seed=4).transpose(2, 0, 1)
    path = str(tmp_path / "r.tif")
    write_geotiff(path, data, T, compression="jpeg", jpeg_quality=95, **layout)
    g = GeoTiff(path)
    assert g.count == 4 and int(g.tags[262][0]) == 2 and list(g.tags[338]) == [0] and 530 not in g.tags    # the GDAL layout of RGBI
    assert (347 in g.tags) == bool(layout.get("jpeg_tables"))
    got = g.read()
    assert got.shape == (4, h, w) and int(np.abs(got.astype(int) - data).max()) <= 12          # quality 95: the bands as written
    g._setup_blocks()
    for by in range(g._ny):                                     # every block as Pillow's libjpeg decodes its rebuilt stream
        for bx in range(g._nx):
            i = by * g._nx + bx
            raw = bytes(g._mm[g._offs[i]:g._offs[i] + g._counts[i]])
            assert (b"Adobe" in raw[:64]) == (not layout.get("jpeg_tables"))
            stream = b"\xff\xd8" + g._jpeg_tables[2:-2] + raw[2:]
            assert_same(stream)
            rows, cols = min(g._block_rows(by), h - by * g._bh), min(g._bw, w - bx * g._bw)
            assert np.array_equal(pillow(stream)[1][:rows, :cols].transpose(2, 0, 1), got[:, by * g._bh:by * g._bh + rows, bx * g._bw:bx * g._bw + cols])
    assert np.array_equal(g._window_hwc(7, 9, 60, 85), got[:, 7:67, 9:94].transpose(1, 2, 0))
    assert g.device_decodable() is True
    info, segs, sets, ncoef = g._jpeg_plan()
    nb = g._nx * g._ny
    assert info.shape == (nb, 8) and (info[:, 0] == 0).all() and (info[:, 2] == 4).all() and (info[:, 3] == 0).all()
    assert (info[:, 4] == g._bw).all() and (info[:, 7] == layout.get("jpeg_restart", 0)).all() and len(sets) == 1
    mcus = -(-info[:, 4] // 8) * -(-info[:, 5] // 8)
    assert ncoef == int((mcus * 4 * 64).sum()) and (np.diff(info[:, 6]) == (mcus * 256)[:-1]).all()
    assert len(segs) == (int(mcus.sum()) if layout.get("jpeg_restart") else nb)
    assert sets.shape[1] == _lib.JPEG_TABSET_BYTES
    g.close()


def _with_block(tmp_path, stream_of):
    """A four-band raster of 32 x 32 tiles whose block 1 is replaced by ``stream_of(block pixels [32, 32, 4])``."""
    path = str(tmp_path / "p.tif")
    data = image(64, 64, "noise", seed=2)
    write_geotiff(path, data.transpose(2, 0, 1), (1, 0, 0, 0, -1, 64), compression="jpeg", tile=(32, 32), jpeg_quality=100)
    g = GeoTiff(path)
    g._setup_blocks()
    off, cnt = g._offs[1], g._counts[1]
    g.close()
    new = stream_of(data[:32, 32:])
    assert len(new) <= cnt
    raw = bytearray(open(path, "rb").read())
    raw[off:off + len(new)] = new
    open(path, "wb").write(bytes(raw))
    return path


def _ycck(stream: bytes) -> bytes:
    at = stream.index(b"Adobe") + 11
    assert stream[at] == 0
    return stream[:at] + b"\x02" + stream[at + 1:]


REFUSED = {"subsampled": lambda blk: encode(255 - blk, quality=60, subsampling=2),
           "ycck": lambda blk: _ycck(encode(255 - blk, quality=60)),
           "progressive": lambda blk: encode(255 - blk, quality=60, progressive=True)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_what_the_decoder_and_the_plan_refuse(tmp_path, what):
    """Other sampling factors, an Adobe segment that names YCCK, progressive: ERR_UNSUPPORTED from td_jpeg_decode, an unsupported block
    in the plan — the raster keeps the host reader."""
    stream = REFUSED[what](image(32, 32, "smooth"))
    assert decode(stream) == _lib.ERR_UNSUPPORTED
    assert b"unsupported" in _lib.load().td_last_error()
    path = _with_block(tmp_path, REFUSED[what])
    g = GeoTiff(path)
    assert g.device_decodable() is False and g._jpeg_plan() is None
    g._setup_blocks()
    lib = _lib.load()
    nb = g._nx * g._ny
    offs, cnts = np.asarray(g._offs, dtype=np.int64), np.asarray(g._counts, dtype=np.int64)
    rows = np.full(nb, 32, dtype=np.int32)
    info, totals = np.zeros((nb, 8), dtype=np.int64), np.zeros(4, dtype=np.int64)
    segs, sets = np.zeros((64, 4), dtype=np.int64), np.zeros((4, _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
    st = lib.td_tiff_jpeg_plan(0, 0, g._mm.ctypes.data, offs.ctypes.data, cnts.ctypes.data, nb, 2, 4, 32, rows.ctypes.data, info.ctypes.data,
                               segs.ctypes.data, len(segs), sets.ctypes.data, len(sets), totals.ctypes.data)
    assert st == 0 and list(info[:, 0]) == [0, 1, 0, 0] and totals[3] == 1 and (info[[0, 2, 3], 2] == 4).all()
    if what == "ycck":
        with pytest.raises(ValueError, match="YCCK"):           # neither reader converts it: refused, not decoded as something else
            g.read()
    elif what == "subsampled":
        assert g.read().shape == (4, 64, 64)                    # the host reader (libjpeg) serves it
    g.close()


def test_a_three_band_plan_refuses_four_component_blocks_and_the_reverse(tmp_path):
    lib = _lib.load()
    for comps, bands in ((4, 3), (3, 4), (4, 1)):
        blk = image(32, 32, "smooth")
        stream = encode(blk, quality=80) if comps == 4 else (lambda b: (Image.fromarray(blk[:, :, :3]).save(b, "JPEG", quality=80), b.getvalue())[1])(io.BytesIO())
        src = np.frombuffer(stream, dtype=np.uint8)
        offs, cnts, rows = np.zeros(1, np.int64), np.array([src.size], np.int64), np.array([32], np.int32)
        info, totals = np.zeros((1, 8), dtype=np.int64), np.zeros(4, dtype=np.int64)
        segs, sets = np.zeros((4, 4), dtype=np.int64), np.zeros((2, _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
        st = lib.td_tiff_jpeg_plan(0, 0, src.ctypes.data, offs.ctypes.data, cnts.ctypes.data, 1, 2, bands, 32, rows.ctypes.data, info.ctypes.data,
                                   segs.ctypes.data, len(segs), sets.ctypes.data, len(sets), totals.ctypes.data)
        assert st == 0 and info[0, 0] == 1 and totals[3] == 1, (comps, bands)


def test_truncated_streams_are_errors():
    stream = encode(image(40, 56, "noise"), quality=90)
    for cut in (len(stream) // 2, len(stream) - 300, len(stream) - 40, 700):
        assert decode(stream[:cut]) < 0
    assert decode(encode(image(40, 56, "noise"), quality=90, restart_marker_blocks=2)[:-500]) < 0


def test_bit_flips_are_errors_or_decode_as_libjpeg_does():
    """A flipped bit in the entropy-coded data of a 40 x 56 stream either decodes as libjpeg decodes it, or is reported: never other
    pixels with status 0 (the rule of the three-band test)."""
    rng = np.random.default_rng(11)
    stream = encode(image(40, 56, "smooth"), quality=90)
    start = stream.index(b"\xff\xda") + 16
    errors = same = 0
    for _ in range(160):
        bad = bytearray(stream)
        pos = int(rng.integers(start, len(stream) - 2))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        got = decode(bytes(bad))
        if isinstance(got, int):
            assert got == _lib.ERR_INVALID
            errors += 1
            continue
        assert np.array_equal(got, pillow(bytes(bad))[1]), pos
        same += 1
    assert errors > 0
    print(f"{errors} flips reported, {same} decoded as libjpeg decodes them")


def test_the_committed_streams_of_the_sanitizer_program_are_what_pillow_decodes():
    """tests/golden/jpeg4 (make_jpeg4_fixture.py): the .raw beside each stream is Pillow's libjpeg decode of it, and td_jpeg_decode's."""
    import glob
    import os
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg4", "*.jpg")))
    assert len(files) == 3
    for f in files:
        stream = open(f, "rb").read()
        assert_same(stream)
        assert pillow(stream)[1].tobytes() == open(f[:-4] + ".raw", "rb").read()
