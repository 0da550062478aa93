"""JPEG-in-TIFF rasters whose entropy-coded segments are decoded by a whole wave each (jpegdecode.hip: jpeg_entropy_sync_kernel +
jpeg_dc_scan_kernel, through GeoTiff.decode_to_device(long_segments=True)) against the host reader (GeoTiff.read: Pillow's libjpeg),
byte for byte: every layout of the lane-per-segment tests with EVERY segment sent through the new kernels (long_threshold=0), segments
of many windows, flat areas (many blocks per subsequence), short and long segments in one call, a corrupt long segment reported by
block, and the Predictor's files unchanged with ``device_decode_long_jpeg`` on or off. None of this makes a kernel fault: corrupt data
is data the decoder reports."""
import json
import os

import numpy as np
import pytest

from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


def _raster(bands, h, w, seed=0):
    rgb, _ = make_tile(seed, max(h, w))
    img = np.concatenate([rgb[:h, :w], rgb[:h, :w, 1:2][:, ::-1]], axis=2)[:, :, :bands]
    img = np.ascontiguousarray(img.transpose(2, 0, 1))
    img[:, h // 5: h // 2, w // 8: w // 2] = 7                      # a flat area
    img[:, -40:, -90:] = np.arange(90, dtype=np.uint8)              # a ramp
    return img


def _busy(bands, h, w, seed=0):
    """The synthetic orthophoto under heavy noise: 256 x 256 blocks of it hold more than JPEG_DEVICE_MAX_SEGMENT bytes at quality 90."""
    rng = np.random.default_rng(seed)
    img = _raster(bands, h, w, seed).astype(np.int16) + rng.integers(-90, 91, (bands, h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def _long_equals_host(path, **kw):
    g = GeoTiff(path)
    assert g.device_decodable(long_segments=True)
    image, check = g.decode_to_device("cuda:0", long_segments=True, **kw)
    got = check().cpu().numpy()
    ref = GeoTiff(path).read()
    assert got.shape == (g.height, g.width, g.count)
    assert np.array_equal(got.transpose(2, 0, 1), ref), int((got.transpose(2, 0, 1) != ref).sum())
    assert check.compressed_bytes > 0 and check.kernel_ms > 0
    if check.long_segments:
        rounds, windows, most, single = check.sync_stats
        assert windows >= check.long_segments and windows <= rounds <= 64 * windows and 1 <= most <= 64 and single <= windows
        assert check.sync_rounds == rounds / windows
    g.close()
    return check


@pytest.mark.parametrize("bands,kw", [(3, {"tile": (128, 256)}), (1, {"tile": (64, 64)}), (3, {"rows_per_strip": 32}),
                                      (1, {"rows_per_strip": 32}), (3, {"tile": (64, 128), "jpeg_tables": True}),
                                      (3, {"rows_per_strip": 48, "jpeg_tables": True, "jpeg_restart": 3}),
                                      (3, {"tile": (128, 128), "jpeg_restart": 1}), (1, {"tile": (32, 48), "jpeg_restart": 2}),
                                      (3, {"tile": (64, 64), "jpeg_subsampling": 0}), (3, {"tile": (64, 64), "jpeg_subsampling": 1, "jpeg_quality": 50}),
                                      (4, {"tile": (64, 64)}), (4, {"rows_per_strip": 16}),
                                      (4, {"tile": (128, 128), "jpeg_restart": 1, "jpeg_tables": True})])
def test_every_segment_through_the_wave_decoder(tmp_path, bands, kw):
    """The layouts of test_jpeg_decode_gpu.py and test_jpeg4_decode_gpu.py with long_threshold=0: tiles padded at the edges, strips
    with a short last strip, shared tables, restart intervals of 1 - 3 MCUs (segments shorter than one subsequence, of one MCU, with
    mcu0 != 0), grey / 4:4:4 / 4:2:2 / 4:2:0 / four bands."""
    path = str(tmp_path / "r.tif")
    write_geotiff(path, _raster(bands, 517, 683, seed=bands), T, 25832, compression="jpeg", **kw)
    check = _long_equals_host(path, long_threshold=0)
    assert check.long_segments == check.segments > 0


@pytest.mark.parametrize("subseq", [32, 128])
def test_one_noise_tile_of_many_windows(tmp_path, subseq):
    """512 x 512 of noise at quality 100, 4:4:4, one segment of several hundred KB: hundreds of windows, blocks longer than a
    subsequence (lanes with no block start of their own), states that travel many lanes before they hold."""
    rng = np.random.default_rng(5)
    path = str(tmp_path / "n.tif")
    write_geotiff(path, rng.integers(0, 256, (3, 512, 512), dtype=np.uint8), T, 25832, compression="jpeg", tile=(512, 512), jpeg_quality=100,
                  jpeg_subsampling=0)
    g = GeoTiff(path)
    assert not g.device_decodable() and int(g._jpeg_plan()[1][0, 1]) > 64 * 128 * 8
    check = _long_equals_host(path, subseq_bytes=subseq)
    assert check.long_segments == 1 and check.sync_stats[1] == -(-int(g._jpeg_plan()[1][0, 1]) // (64 * subseq))
    assert check.sync_stats[2] > 2 and check.sync_rounds > 1.0
    # the tile is one complete stream of one segment: the wave counts what the host emulation of its 64 lanes counts (treedet.h)
    src = np.array(g._mm[g._offs[0]:g._offs[0] + g._counts[0]], dtype=np.uint8)
    out, shape, stats = np.zeros(512 * 512 * 3, dtype=np.uint8), np.zeros(3, dtype=np.int32), np.zeros(4, dtype=np.int64)
    n = _lib.load().td_jpeg_decode_sync(src.ctypes.data, src.size, out.ctypes.data, out.size, shape.ctypes.data, subseq, 64, stats.ctypes.data)
    assert n == out.size and list(check.sync_stats) == [int(v) for v in stats], (check.sync_stats, stats)


def test_half_flat_half_noise(tmp_path):
    """Flat blocks are a handful of bits each: tens of blocks per subsequence, whose counts the prefix sum turns into block ordinals."""
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (3, 517, 683), dtype=np.uint8)
    img[:, :, :340] = 120
    for kw in ({"tile": (256, 256)}, {"rows_per_strip": 64, "jpeg_subsampling": 0}):
        path = str(tmp_path / f"h{len(kw)}.tif")
        write_geotiff(path, img, T, 25832, compression="jpeg", **kw)
        _long_equals_host(path, long_threshold=0)


def test_short_and_long_segments_in_one_call(tmp_path):
    """The default threshold and subsequence size: the flat tiles stay with the lane-per-segment kernel, the noise tiles take a wave each."""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (3, 517, 683), dtype=np.uint8)
    img[:, :, :300] = 120
    path = str(tmp_path / "m.tif")
    write_geotiff(path, img, T, 25832, compression="jpeg", tile=(256, 256))
    g = GeoTiff(path)
    assert not g.device_decodable()
    nbytes = g._jpeg_plan()[1][:, 1]
    nlong = int((nbytes > GeoTiff.JPEG_DEVICE_MAX_SEGMENT).sum())
    assert 0 < nlong < len(nbytes)
    check = _long_equals_host(path)
    assert check.long_segments == nlong and check.segments == len(nbytes)


def _predict(tmp_path, tag, tif, long_jpeg, calls, capsys=None):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    d = tmp_path / tag
    name = os.path.splitext(os.path.basename(tif))[0]
    tile_single_file(tif, str(d / "tiles"), buffer=10, tile_width=40, tile_height=40)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    with TD.Predictor(cfg, device_type="0", max_batch_size=3, output_dir=str(d / "out"), state_dict=sd,
                      device_decode_long_jpeg=long_jpeg) as pred:
        for _ in range(calls):
            pred.prefetch(tif)
            pred(tif, str(d / "tiles" / f"{name}.json"))
        images = pred.decode_stats["images"]
    files = sorted(os.listdir(d / "out" / name))
    return images, {f: open(d / "out" / name / f, "rb").read().replace(tif.encode(), b"IMG") for f in files}


def test_a_corrupt_long_segment_is_reported_and_the_predictor_falls_back(tmp_path, capsys):
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, _busy(3, 300, 500, seed=9), T, 25832, compression="jpeg", tile=(256, 256))
    g = GeoTiff(good)
    g._setup_blocks()
    raw = bytearray(open(good, "rb").read())
    off, cnt = g._offs[1], g._counts[1]
    g.close()
    assert cnt > GeoTiff.JPEG_DEVICE_MAX_SEGMENT
    sos = raw.index(b"\xff\xda", off)
    mid = sos + (off + cnt - sos) // 2
    raw[mid:mid + 16] = b"\xff\x00" * 8                             # all-ones bits: no code of the tables, in the middle of block 1
    open(bad, "wb").write(bytes(raw))
    gb = GeoTiff(bad)
    assert gb.device_decodable(long_segments=True) and not gb.device_decodable()
    image, check = gb.decode_to_device("cuda:0", long_segments=True)
    with pytest.raises(ValueError, match="block 1 "):
        check()
    gb.close()
    capsys.readouterr()
    on, files_on = _predict(tmp_path, "on", bad, True, 1)
    assert "using the host reader" in capsys.readouterr().out and on == 0
    off_, files_off = _predict(tmp_path, "off", bad, False, 1)
    assert "using the host reader" not in capsys.readouterr().out and off_ == 0
    assert len(files_on) >= 4 and files_on == files_off


def test_prediction_files_are_identical_with_the_long_jpeg_key_on_or_off(tmp_path):
    """A 4:2:0 raster of 256 x 256 tiles without restart markers through the Predictor twice (the second time prefetched): windows cut in
    HBM from the wave-per-segment decode (key on) against the host reader, which serves it with the key off."""
    tif = str(tmp_path / "9.tif")
    write_geotiff(tif, _busy(3, 300, 500, seed=300), T, 25832, compression="jpeg", tile=(256, 256))
    g = GeoTiff(tif)
    assert not g.device_decodable() and g.device_decodable(long_segments=True)
    g.close()
    on, files_on = _predict(tmp_path, "on", tif, True, 2)
    off, files_off = _predict(tmp_path, "off", tif, False, 2)
    assert (on, off) == (2, 0)
    assert len(files_on) >= 4 and files_on == files_off
    assert sum(len(json.loads(v)) for v in files_on.values()) > 0
