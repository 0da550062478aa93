"""Band-separate (PlanarConfiguration = 2) rasters and the device decoders, the parts that need no GPU: which files
``GeoTiff.device_decodable(planar=True)`` admits (and that every answer without the keyword is what it was), the block plan of a band
subset, the ``device_decode_planar`` setting as the Predictor and the crown stage read it, and the three td_tiff_planes_to_image*_dev
entry points: declared, exported, bound, and refusing bad arguments before anything is launched."""
import os
import struct
import zlib

import numpy as np
import pytest

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P
from treedetection_amd.device_decode import stage_offsets
from treedetection_amd.geotiff import GeoTiff, device_decode_planar_setting, write_geotiff

from f32_cases import to_big_endian

T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("td_tiff_planes_to_image_dev", "td_tiff_planes_to_image_u16_dev", "td_tiff_planes_to_image_f32_dev")


def _image(bands, dtype, h=61, w=83, seed=1):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.normal(10.0, 3.0, (bands, h, w)).astype(dtype)
    return rng.integers(0, np.iinfo(dtype).max, (bands, h, w), dtype=dtype)


@pytest.mark.parametrize("codec", ["lzw", "deflate"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("kw", [{"tile": (32, 48), "predictor": 2}, {"rows_per_strip": 9}])
def test_planar_integer_files_qualify_only_when_asked(tmp_path, codec, dtype, kw):
    path = str(tmp_path / "p.tif")
    write_geotiff(path, _image(3, dtype), T, 25832, compression=codec, planar=True, **kw)
    g = GeoTiff(path)
    assert g.planar == 2
    assert g.device_decodable(planar=True) is True
    assert g.device_decodable() is False and g.device_decodable(planar=False) is False
    assert g.device_uploadable() is False


@pytest.mark.parametrize("predictor", [1, 2, 3])
def test_planar_float32_needs_float_samples_too(tmp_path, predictor):
    path = str(tmp_path / "f.tif")
    write_geotiff(path, _image(2, np.float32), T, 25832, compression="deflate", planar=True, predictor=predictor, tile=(32, 32))
    g = GeoTiff(path)
    assert g.device_decodable(planar=True, float_samples=True) is True
    assert g.device_decodable(planar=True) is False
    assert g.device_decodable(float_samples=True) is False


def test_a_chunky_files_answers_do_not_depend_on_planar(tmp_path):
    for name, dtype, kw in (("lzw8", np.uint8, {"compression": "lzw", "tile": (32, 48), "predictor": 2}), ("raw8", np.uint8, {}),
                            ("deflate16", np.uint16, {"compression": "deflate", "rows_per_strip": 9}),
                            ("f32", np.float32, {"compression": "lzw", "predictor": 3})):
        path = str(tmp_path / f"{name}.tif")
        write_geotiff(path, _image(3, dtype), T, 25832, **kw)
        g = GeoTiff(path)
        for fs in (False, True):
            assert g.device_decodable(float_samples=fs, planar=True) == g.device_decodable(float_samples=fs), (name, fs)
    assert GeoTiff(str(tmp_path / "lzw8.tif")).device_decodable(planar=True) is True
    assert GeoTiff(str(tmp_path / "raw8.tif")).device_decodable(planar=True) is False


def _set_short_tag(path, tag, value):
    """Overwrites the inline SHORT value of ``tag`` in the first IFD of a little-endian classic TIFF."""
    raw = bytearray(open(path, "rb").read())
    assert raw[:4] == b"II*\0"
    ifd = struct.unpack("<I", raw[4:8])[0]
    for i in range(struct.unpack("<H", raw[ifd:ifd + 2])[0]):
        e = ifd + 2 + 12 * i
        t, typ, cnt = struct.unpack("<HHI", raw[e:e + 8])
        if t == tag:
            assert typ == 3 and cnt == 1
            raw[e + 8:e + 10] = struct.pack("<H", value)
            open(path, "wb").write(bytes(raw))
            return
    raise AssertionError(f"tag {tag} not in {path}")


def test_big_endian_planar_and_planar_jpeg_answer_false_either_way(tmp_path):
    le, be, jp = (str(tmp_path / n) for n in ("le.tif", "be.tif", "jpeg.tif"))
    write_geotiff(le, _image(3, np.uint16), T, 25832, compression="lzw", planar=True, rows_per_strip=9)
    to_big_endian(le, be)
    assert open(be, "rb").read(2) == b"MM" and GeoTiff(be).dtype.byteorder == ">" and GeoTiff(be).planar == 2
    write_geotiff(jp, _image(1, np.uint8, 64, 64), T, 25832, compression="jpeg", tile=(32, 32))
    assert GeoTiff(jp).device_decodable()
    _set_short_tag(jp, 284, 2)                              # one band, declared band-separate: the same bytes, a planar JPEG file
    assert GeoTiff(jp).planar == 2 and GeoTiff(jp).compression == 7
    for path in (be, jp):
        for planar in (False, True):
            assert GeoTiff(path).device_decodable(planar=planar, float_samples=True, long_segments=True) is False, (path, planar)


def test_the_block_plan_of_a_band_subset(tmp_path):
    """4 bands, 157 rows in strips of 7: 23 strips per plane, the last one of 3 rows."""
    path = str(tmp_path / "p.tif")
    img = _image(4, np.uint8, 157, 83)
    write_geotiff(path, img, T, 25832, compression="lzw", planar=True, rows_per_strip=7, predictor=2)
    g = GeoTiff(path)
    g._setup_blocks()
    assert len(g._offs) == 4 * 23
    planes, mask, offs, cnts, expect, ranges = g.device_block_plan(bands=(0, 3))
    assert planes == [0, 3] and mask == 0b1001
    assert offs.dtype == np.int64 and cnts.dtype == np.int64 and expect.dtype == np.int64
    assert offs.tolist() == g._offs[0:23] + g._offs[69:92] and cnts.tolist() == g._counts[0:23] + g._counts[69:92]
    assert expect.tolist() == ([7 * 83] * 22 + [3 * 83]) * 2
    # what is read: the two planes' own bytes, nothing of planes 1 and 2
    assert ranges == [(g._offs[0], g._offs[22] + g._counts[22]), (g._offs[69], g._offs[91] + g._counts[91])]
    assert int(cnts.sum()) <= sum(hi - lo for lo, hi in ranges) < int(cnts.sum()) + len(cnts)     # (the writer begins a block at an even offset)
    # any order of the bands, the same plan; all bands: one range again, every block
    assert g.device_block_plan(bands=[3, 0])[0] == [0, 3]
    planes, mask, offs, cnts, expect, ranges = g.device_block_plan()
    assert planes == [0, 1, 2, 3] and mask == 0b1111 and offs.tolist() == g._offs and len(ranges) == 1 and len(expect) == 92
    for bad in ((), (4,), (-1,), (0, 0)):
        with pytest.raises(ValueError, match="bands"):
            g.device_block_plan(bands=bad)
    # uint16: the sizes count bytes
    write_geotiff(path, _image(2, np.uint16, 157, 83), T, 25832, compression="deflate", planar=True, rows_per_strip=7)
    assert GeoTiff(path).device_block_plan(bands=(1,))[4].tolist() == [7 * 83 * 2] * 22 + [3 * 83 * 2]
    # a pixel-interleaved file: one plane that holds every band, and no subset
    write_geotiff(path, img, T, 25832, compression="lzw", rows_per_strip=7)
    c = GeoTiff(path)
    planes, mask, offs, cnts, expect, ranges = c.device_block_plan()
    assert planes == [0] and mask == 1 and expect.tolist() == [7 * 83 * 4] * 22 + [3 * 83 * 4] and len(ranges) == 1
    with pytest.raises(ValueError, match="bands"):
        c.device_block_plan(bands=(0, 3))


def test_staged_blocks_lie_where_stage_offsets_says(tmp_path):
    """The byte ranges of the plan, one behind the other as decode_to_device stages them: every block's stream begins at its ``rel``
    (zlib inflates it to the block's size from there), and ``span`` is all that is staged."""
    path = str(tmp_path / "p.tif")
    img = np.random.default_rng(0).integers(0, 256, (4, 80, 112), dtype=np.uint8)
    # (band-separate or not, bands) → ranges, blocks: 3 x 3 tiles per plane
    for planar, bands, nranges, nb in ((True, (0, 3), 2, 18), (True, None, 1, 36), (False, None, 1, 9)):
        write_geotiff(path, img, T, 25832, compression="deflate", planar=planar, tile=(32, 48))
        planes, mask, offs, cnts, expect, ranges = GeoTiff(path).device_block_plan(bands)
        assert len(ranges) == nranges and len(offs) == nb, (planar, bands, ranges)
        rel, starts, span = stage_offsets(offs, ranges)
        raw = open(path, "rb").read()
        staged = b"".join(raw[lo:hi] for lo, hi in ranges)
        assert span == len(staged) == sum(hi - lo for lo, hi in ranges)
        assert starts.tolist() == np.cumsum([0] + [hi - lo for lo, hi in ranges]).tolist()
        for i in range(nb):
            assert 0 <= rel[i] and rel[i] + cnts[i] <= span
            block = zlib.decompress(staged[rel[i]:rel[i] + cnts[i]])
            assert len(block) == expect[i], (planar, bands, i)
            # ... and it is THAT block: plane i // 9 of the selected ones, tile (i % 9 // 3, i % 3), its pixels inside the raster
            by, bx = i % 9 // 3, i % 3
            want = img[planes[i // 9]:planes[i // 9] + 1] if planar else img
            want = want[:, by * 32:(by + 1) * 32, bx * 48:(bx + 1) * 48].transpose(1, 2, 0)
            got = np.frombuffer(block, np.uint8).reshape(32, 48, -1)[:want.shape[0], :want.shape[1]]
            assert np.array_equal(got, want), (planar, bands, i)


def test_the_setting_is_read_alike_and_refuses_anything_else():
    import treedetection_amd as TD
    assert device_decode_planar_setting() is False and device_decode_planar_setting(None) is False
    assert device_decode_planar_setting(True) is True and device_decode_planar_setting("true") is True
    assert device_decode_planar_setting(False) is False and device_decode_planar_setting("false") is False
    for bad in ("auto", "all", 1, 0, "yes", "True"):
        with pytest.raises(ValueError, match="device_decode_planar"):
            device_decode_planar_setting(bad)
        with pytest.raises(ValueError, match="device_decode_planar"):
            P._planar_on({"device_decode_planar": bad})
        with pytest.raises(ValueError, match="device_decode_planar"):
            TD.Predictor(None, device_decode_planar=bad)
    assert P._planar_on({}) is False and P._planar_on({"device_decode_planar": "true"}) is True
    assert P._planar_on({"device_decode_planar": False}) is False
    assert "device_decode_planar: false" in open(os.path.join(ROOT, "example", "config.yml")).read()


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "treedet.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert f"td_status {name}(" in header, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 13, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name


@pytest.mark.parametrize("name,item", list(zip(NAMES, (1, 2, 4))))
def test_bad_arguments_are_refused_before_any_launch(name, item):
    """No GPU here and no memory behind the pointers: every one of these calls has to return from its checks."""
    fn = getattr(_lib.load(), name)
    ptr = 1 << 20
    ok = dict(blocks=ptr, block_cap=16 * 8 * item, block_w=16, block_h=8, blocks_across=2, blocks_down=3, spp=4, plane_mask=0b1001,
              predictor=2, image=ptr, width=30, height=20, stream=None)
    cases = {"spp": (dict(spp=5), "samples per pixel"), "no plane": (dict(plane_mask=0), "plane mask"),
             "a plane beyond spp": (dict(plane_mask=0b10001), "plane mask"), "a plane beyond spp 2": (dict(spp=2, plane_mask=0b100), "plane mask"),
             "block_cap": (dict(block_cap=16 * 8 * item - item), "does not fit"), "geometry": (dict(blocks_across=3), "do not tile"),
             "null": (dict(blocks=None), "null pointer"), "columns": (dict(blocks_across=65536, width=65536 * 16), "block columns"),
             "predictor": (dict(predictor=4), "predictor 4")}
    if item == 1:
        cases["predictor 3 on uint8"] = (dict(predictor=3), "predictor 3")
    if item == 2:
        cases["predictor 3 on uint16"] = (dict(predictor=3), "predictor 3")
    if item > 1:
        cases["alignment"] = (dict(blocks=ptr + 1), "multiples of the sample size")
        cases["block_cap alignment"] = (dict(block_cap=16 * 8 * item + 1), "multiples of the sample size")
    for what, (change, message) in cases.items():
        args = dict(ok, **change)
        assert fn(*args.values()) == _lib.ERR_INVALID, what
        text = _lib.load().td_last_error().decode()
        assert text.startswith(name + ":") and message in text, (what, text)
