"""The JPEG decoder of jpeg_core.h on one host thread (td_jpeg_decode) against Pillow's libjpeg, byte for byte — the decoder the GPU
runs for JPEG-in-TIFF rasters (jpegdecode.hip) — and the host plan (td_tiff_jpeg_plan) on the writer's and libtiff's TIFFs."""
import io

import numpy as np
import pytest
from PIL import Image, ImageFile

from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, _jpeg_split, write_geotiff

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def decode(stream: bytes):
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8)
    out = np.zeros(1 << 22, dtype=np.uint8)
    shape = np.zeros(3, dtype=np.int32)
    n = lib.td_jpeg_decode(src.ctypes.data, src.size, out.ctypes.data, out.size, shape.ctypes.data)
    if n < 0:
        return n
    h, w, c = (int(v) for v in shape)
    assert n == h * w * c
    arr = out[:n].reshape(h, w, c)
    return arr[:, :, 0] if c == 1 else arr


def encode(img: np.ndarray, mode: str, **kw) -> bytes:
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24                   # optimize=True on noise needs the whole stream in one buffer
    try:
        buf = io.BytesIO()
        if mode == "L":
            Image.fromarray(img[:, :, 0]).save(buf, "JPEG", **kw)
        else:
            Image.fromarray(img).save(buf, "JPEG", subsampling=SUBSAMPLING[mode], **kw)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def pillow(stream: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(stream)) as im:
        return np.asarray(im)


def image(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def assert_same(stream: bytes):
    ref = pillow(stream)
    got = decode(stream)
    assert not isinstance(got, int), f"td_jpeg_decode returned {got}: {_lib.load().td_last_error()}"
    assert got.shape == ref.shape and np.array_equal(got, ref), (got.shape, ref.shape, int((got != ref).sum()))


@pytest.mark.parametrize("mode", ["L", "444", "422", "420"])
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("size", [(1, 1), (7, 13), (17, 33), (517, 683)])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_matches_pillow(mode, quality, size, kind):
    assert_same(encode(image(*size, kind), mode, quality=quality))


@pytest.mark.parametrize("mode", ["L", "444", "422", "420"])
@pytest.mark.parametrize("opts", [{"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1},
                                  {"restart_marker_blocks": 5, "optimize": True}])
def test_optimized_tables_and_restart_intervals(mode, opts):
    for kind in ("noise", "smooth"):
        assert_same(encode(image(71, 133, kind, seed=3), mode, quality=90, **opts))


@pytest.mark.parametrize("mode", ["L", "444", "422", "420"])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_large_quantisation_steps_exercise_range_limiting(mode, kind):
    """Steps of 255 make the IDCT overshoot far beyond 0..255: the decoder's range-limit table (clamp, then its wrap-around)."""
    for qt in ([[255] * 64, [255] * 64], [[1] + [200] * 63, [255] * 64], [[2] * 64, [255] * 64]):
        stream = encode(image(64, 96, kind, seed=5), mode, qtables=qt[:1] if mode == "L" else qt)
        assert_same(stream)


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (3, 5), (5, 4), (9, 2), (33, 1)])
@pytest.mark.parametrize("mode", ["422", "420"])
def test_narrow_and_short_images(size, mode):
    """Chroma components of 1 - 2 samples (libjpeg replicates them instead of filtering) and single rows / columns."""
    assert_same(encode(image(*size, "noise", seed=size[0] * 7 + size[1]), mode, quality=85))


@pytest.mark.parametrize("mode", ["L", "420"])
def test_abbreviated_stream_with_tables_split_off(mode):
    """A block without its tables (the GDAL / libtiff layout): tables minus EOI + block minus SOI is one complete stream."""
    tables, block = _jpeg_split(encode(image(48, 80, "smooth"), mode, quality=75))
    assert b"\xff\xdb" not in block[:block.index(b"\xff\xda")] and b"JFIF" not in block
    assert decode(block) == _lib.ERR_UNSUPPORTED                # no tables of its own
    assert_same(tables[:-2] + block[2:])


def test_libtiff_written_tiffs(tmp_path):
    """Pillow's TIFF writer through libtiff (JPEGTables + abbreviated strips): every strip, rebuilt as the host reader builds it,
    decodes as Pillow decodes it, and the plan accepts the raster."""
    rgb = image(80, 120, "smooth", seed=9)
    for data, name in ((rgb, "rgb"), (rgb[:, :, 0], "grey")):
        path = str(tmp_path / f"{name}.tif")
        Image.fromarray(data).save(path, compression="jpeg", quality=80)
        g = GeoTiff(path)
        assert g.compression == 7
        g._setup_blocks()
        assert g.device_decodable() is True
        for by in range(g._ny):
            raw = bytes(g._mm[g._offs[by]:g._offs[by] + g._counts[by]])
            stream = b"\xff\xd8"
            if g.count == 3 and b"JFIF\0" not in raw[:32]:
                stream += b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + (b"\x01" if int(g.tags[262][0]) == 6 else b"\x00")
            stream += g._jpeg_tables[2:-2] + raw[2:]
            assert_same(stream)
        g.close()


def test_progressive_is_unsupported():
    stream = encode(image(40, 40, "smooth"), "420", quality=90, progressive=True)
    assert decode(stream) == _lib.ERR_UNSUPPORTED
    assert b"unsupported" in _lib.load().td_last_error()


def test_truncated_streams_are_errors():
    stream = encode(image(96, 128, "noise"), "420", quality=90)
    for cut in (len(stream) // 2, len(stream) - 300, len(stream) - 40, 700):
        assert decode(stream[:cut]) < 0
    assert decode(encode(image(96, 128, "noise"), "420", quality=90, restart_marker_blocks=2)[:-500]) < 0


def test_bit_flips_are_errors_or_decode_as_libjpeg_does():
    """A flipped bit in the entropy-coded data either decodes as libjpeg decodes it, or is reported: never other pixels with status 0."""
    rng = np.random.default_rng(11)
    stream = encode(image(96, 128, "smooth"), "420", quality=90)
    start = stream.index(b"\xff\xda") + 14
    errors = 0
    for _ in range(120):
        bad = bytearray(stream)
        pos = int(rng.integers(start, len(stream) - 2))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        got = decode(bytes(bad))
        if isinstance(got, int):
            assert got == _lib.ERR_INVALID
            errors += 1
            continue
        assert np.array_equal(got, pillow(bytes(bad))), pos
    assert errors > 0


def test_corrupt_huffman_code_run_and_restart_sequence():
    stream = encode(image(32, 32, "noise"), "L", quality=90, restart_marker_blocks=1)
    sos = stream.index(b"\xff\xda")
    data = bytearray(stream)
    rst = data.index(b"\xff\xd0", sos)
    data[rst + 1] = 0xD3                                       # RST3 where RST0 belongs
    assert decode(bytes(data)) == _lib.ERR_INVALID
    ones = bytearray(stream)
    ones[sos + 10:sos + 20] = b"\xff\x00" * 5                  # all-ones bits: not a code of the standard tables
    assert decode(bytes(ones)) < 0


def plan(g: GeoTiff):
    assert g.device_decodable()
    return g._jpeg_plan()


@pytest.mark.parametrize("layout", [dict(tile=(128, 256)), dict(rows_per_strip=32), dict(tile=(64, 64), jpeg_tables=True),
                                    dict(rows_per_strip=48, jpeg_tables=True, jpeg_restart=2), dict(tile=(32, 48), jpeg_restart=1)])
@pytest.mark.parametrize("bands", [1, 3])
def test_plan_of_the_writers_tiffs(tmp_path, layout, bands):
    data = image(517, 683, "smooth").transpose(2, 0, 1)[:bands]
    path = str(tmp_path / "r.tif")
    write_geotiff(path, data, (0.5, 0, 100, 0, -0.5, 200), compression="jpeg", **layout)
    g = GeoTiff(path)
    info, segs, sets, ncoef = plan(g)
    nb = g._nx * g._ny
    assert info.shape == (nb, 8) and (info[:, 0] == 0).all() and len(sets) == 1 and (info[:, 1] == 0).all()
    assert (info[:, 2] == (3 if bands == 3 else 0)).all() and (info[:, 3] == (bands == 3)).all() and (info[:, 4] == g._bw).all()
    rows = np.array([g._block_rows(by) for by in range(g._ny) for _ in range(g._nx)])
    assert (info[:, 5] >= rows).all()
    assert (np.diff(info[:, 6]) > 0).all() and info[0, 6] == 0 and ncoef > info[-1, 6]
    restart = layout.get("jpeg_restart", 0)
    assert (info[:, 7] == restart).all()
    assert (segs[:, 2] == np.repeat(np.arange(nb), np.bincount(segs[:, 2], minlength=nb))).all()
    if not restart:
        assert len(segs) == nb
    else:
        assert len(segs) > nb and ((segs[:, 3] >> 32) <= restart).all()
    offs, cnts = np.asarray(g._offs), np.asarray(g._counts)
    b = segs[:, 2]
    assert (segs[:, 0] >= offs[b]).all() and (segs[:, 0] + segs[:, 1] <= offs[b] + cnts[b]).all()
    assert g.read().shape == (bands, 517, 683)
    g.close()


def test_plan_refuses_progressive_blocks(tmp_path):
    path = str(tmp_path / "p.tif")
    data = image(64, 64, "smooth").transpose(2, 0, 1)
    write_geotiff(path, data, (1, 0, 0, 0, -1, 64), compression="jpeg", tile=(32, 32))
    raw = bytearray(open(path, "rb").read())
    g = GeoTiff(path)
    g._setup_blocks()
    off, cnt = g._offs[1], g._counts[1]
    g.close()
    prog = encode(image(32, 32, "smooth"), "420", quality=90, progressive=True)
    assert len(prog) <= cnt
    raw[off:off + len(prog)] = prog
    open(path, "wb").write(bytes(raw))
    g = GeoTiff(path)
    assert g.device_decodable() is False
    g.close()


def test_rasters_with_segments_beyond_the_lane_limit_stay_on_the_host(tmp_path):
    """One lane decodes one segment serially: a raster whose blocks hold more than JPEG_DEVICE_MAX_SEGMENT bytes without a restart
    marker is left to the host reader; the same pixels with restart intervals go to the device."""
    data = image(1024, 1024, "noise").transpose(2, 0, 1)
    one, cut = str(tmp_path / "one.tif"), str(tmp_path / "cut.tif")
    write_geotiff(one, data, (1, 0, 0, 0, -1, 1024), compression="jpeg", rows_per_strip=1024)
    write_geotiff(cut, data, (1, 0, 0, 0, -1, 1024), compression="jpeg", rows_per_strip=1024, jpeg_restart=16)
    g1, g2 = GeoTiff(one), GeoTiff(cut)
    g1._setup_blocks()
    assert g1._counts[0] > GeoTiff.JPEG_DEVICE_MAX_SEGMENT
    assert g1._jpeg_plan() is not None and g1.device_decodable() is False
    assert g2.device_decodable() is True and int(g2._jpeg_plan()[1][:, 1].max()) <= GeoTiff.JPEG_DEVICE_MAX_SEGMENT
