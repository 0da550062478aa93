"""uint32 rasters (crown label rasters) through write_geotiff → GeoTiff.read: SampleFormat 1, 32 bits; strips and tiles,
uncompressed / LZW / DEFLATE, predictor 1 and 2 (differences of 32-bit words modulo 2^32); what is refused; one file read back
with Pillow."""
import itertools

import numpy as np
import pytest

from treedetection_amd.geotiff import GeoTiff, write_geotiff

T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)
ROWS, COLS = 45, 83                                          # no multiple of the 16 x 32 tiles or of the 7-row strips


def _raster():
    """The four corner values in every neighbourhood the predictor sees (each followed by each), then seeded words."""
    special = np.array([0, 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    pairs = np.array(list(itertools.product(special, special)), dtype=np.uint64).reshape(-1)
    rng = np.random.default_rng(41)
    a = rng.integers(0, 1 << 32, ROWS * COLS, dtype=np.uint64)
    a[:pairs.size] = pairs
    a[-special.size:] = special[::-1]
    a[COLS - 1::COLS][:4] = special                          # and in the last column, where a tile is cut
    return a.astype(np.uint32).reshape(ROWS, COLS)


@pytest.mark.parametrize("layout", ["strip", "strips", "tiles"])
@pytest.mark.parametrize("compression", [None, "lzw", "deflate"])
@pytest.mark.parametrize("predictor", [1, 2])
def test_uint32_round_trip(tmp_path, layout, compression, predictor):
    want = _raster()
    path = str(tmp_path / "labels.tif")
    kw = {"strip": {}, "strips": {"rows_per_strip": 7}, "tiles": {"tile": (16, 32)}}[layout]
    write_geotiff(path, want, T, 25832, compression=compression, predictor=predictor, nodata=0, **kw)
    g = GeoTiff(path)
    assert g.dtype == np.uint32 and (g.height, g.width, g.count) == (ROWS, COLS, 1) and g.nodata == 0.0 and g.epsg == 25832
    assert g.transform == T
    got = g.read()
    g.close()
    assert got.dtype == np.uint32 and got.shape == (1, ROWS, COLS)
    assert np.array_equal(got[0], want)
    assert {0, 1, 1 << 31, (1 << 32) - 1} <= set(got[0].reshape(-1).tolist())


def test_two_bands_and_the_header_fields(tmp_path):
    want = np.stack([_raster(), _raster()[::-1]])
    path = str(tmp_path / "two.tif")
    write_geotiff(path, want, T, 25832, compression="lzw", predictor=2, tile=(32, 32))
    g = GeoTiff(path)
    got = g.read()
    g.close()
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    import struct
    raw = open(path, "rb").read()
    n = struct.unpack_from("<H", raw, 8)[0]
    tags = {struct.unpack_from("<H", raw, 10 + 12 * k)[0]: struct.unpack_from("<HIHH", raw, 12 + 12 * k) for k in range(n)}
    assert tags[258][2:] == (32, 32) and tags[339][2:] == (1, 1)          # BitsPerSample 32, SampleFormat 1 (unsigned), inline for two bands


def test_refusals(tmp_path):
    path = str(tmp_path / "no.tif")
    a = _raster()
    with pytest.raises(ValueError, match="jpeg"):
        write_geotiff(path, a[:32, :32], T, compression="jpeg", tile=(16, 16))
    with pytest.raises(ValueError, match="predictor 3"):
        write_geotiff(path, a, T, compression="deflate", predictor=3)
    with pytest.raises(ValueError, match="predictor must be"):
        write_geotiff(path, a, T, predictor=4)
    with pytest.raises(KeyError):
        write_geotiff(path, a.astype(np.uint64), T)
    import os
    assert not os.path.exists(path)


def test_pillow_reads_the_file(tmp_path):
    """Which way it went where this was written: Pillow opens the 32-bit unsigned TIFF as mode "I" (numpy int32, the same bits),
    and the pixels are compared. A Pillow whose format table lacks the entry refuses the file; the test then says so and compares
    nothing — the round trip above does not depend on Pillow."""
    from PIL import Image
    want = _raster()
    path = str(tmp_path / "pil.tif")
    write_geotiff(path, want, T, 25832, nodata=0)            # one uncompressed strip: the layout Pillow's raw decoder takes
    try:
        with Image.open(path) as im:
            mode = im.mode
            got = np.array(im)
    except Exception as e:                                   # (UnidentifiedImageError, or a decoder that lacks the raw mode)
        print(f"Pillow does not open 32-bit unsigned TIFFs here ({type(e).__name__}: {e}): not compared")
        return
    print(f"Pillow opened the uint32 TIFF as mode {mode!r}, dtype {got.dtype}: compared")
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64) & 0xFFFFFFFF, want.astype(np.int64))
