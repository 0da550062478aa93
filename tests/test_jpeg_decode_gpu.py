"""JPEG-in-TIFF rasters decoded on the GPU (jpegdecode.hip, planned by td_tiff_jpeg_plan) against the host reader (GeoTiff.read: Pillow's
libjpeg block by block): the same bytes for every layout the reader takes, corrupt blocks reported by name, and the Predictor's files
unchanged with the device decoder on or off."""
import json
import os

import numpy as np
import pytest

from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


def _raster(bands, h, w, seed=0):
    rgb, _ = make_tile(seed, max(h, w))
    img = np.ascontiguousarray(rgb[:h, :w, :bands].transpose(2, 0, 1))
    img[:, h // 5: h // 2, w // 8: w // 2] = 7                      # a flat area
    img[:, -40:, -90:] = np.arange(90, dtype=np.uint8)              # a ramp
    return img


def _device_equals_host(path, segments_at_least=0):
    g = GeoTiff(path)
    assert g.device_decodable()
    image, check = g.decode_to_device("cuda:0")
    got = check().cpu().numpy()
    ref = GeoTiff(path).read()
    assert got.shape == (g.height, g.width, g.count)
    assert np.array_equal(got.transpose(2, 0, 1), ref), int((got.transpose(2, 0, 1) != ref).sum())
    assert check.compressed_bytes > 0 and check.kernel_ms > 0 and check.segments >= segments_at_least
    g.close()
    return got


@pytest.mark.parametrize("bands,kw", [(3, {"tile": (128, 256)}), (1, {"tile": (64, 64)}), (3, {"rows_per_strip": 32}),
                                      (1, {"rows_per_strip": 32}), (3, {"tile": (64, 128), "jpeg_tables": True}),
                                      (3, {"rows_per_strip": 48, "jpeg_tables": True, "jpeg_restart": 3}),
                                      (3, {"tile": (128, 128), "jpeg_restart": 1}), (1, {"tile": (32, 48), "jpeg_restart": 2}),
                                      (3, {"tile": (64, 64), "jpeg_subsampling": 0}), (3, {"tile": (64, 64), "jpeg_subsampling": 1, "jpeg_quality": 50})])
def test_device_decode_equals_the_host_reader(tmp_path, bands, kw):
    """Tiles (padded at the right and bottom edges), strips of 32 rows with a 5-row last strip (517 rows), the GDAL layout with shared
    tables, restart intervals, 4:4:4 / 4:2:2 / 4:2:0 and grey."""
    path = str(tmp_path / "r.tif")
    write_geotiff(path, _raster(bands, 517, 683, seed=bands), T, 25832, compression="jpeg", **kw)
    _device_equals_host(path)


def test_device_decode_of_files_written_by_libtiff(tmp_path):
    from PIL import Image
    rgb, _ = make_tile(4, 300)
    for data, name in ((rgb[:233, :300], "rgb"), (rgb[:233, :300, 1], "grey")):
        path = str(tmp_path / f"{name}.tif")
        Image.fromarray(np.ascontiguousarray(data)).save(path, compression="jpeg", quality=85)
        assert GeoTiff(path).compression == 7
        _device_equals_host(path)


def test_more_segments_than_one_round_of_waves_go_by_ticket(tmp_path):
    """A restart marker every MCU: 102 400 segments, more than the 256 workgroups of four 64-lane waves take in one round."""
    rgb, _ = make_tile(6, 2100)
    path = str(tmp_path / "big.tif")
    write_geotiff(path, rgb[:, :, 0], T, 25832, compression="jpeg", tile=(512, 512), jpeg_restart=1)
    _device_equals_host(path, segments_at_least=100000)


def test_a_corrupt_block_is_reported_and_the_predictor_falls_back(tmp_path, capsys):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    img = _raster(3, 500, 500, seed=9)
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, img, T, 25832, compression="jpeg", tile=(128, 128))
    g = GeoTiff(good)
    g._setup_blocks()
    raw = bytearray(open(good, "rb").read())
    off, cnt = g._offs[5], g._counts[5]
    sos = raw.index(b"\xff\xda", off)
    mid = sos + (off + cnt - sos) // 2
    raw[mid:mid + 16] = b"\xff\x00" * 8                             # all-ones bits: no code of the tables in block 5
    open(bad, "wb").write(bytes(raw))
    gb = GeoTiff(bad)
    assert gb.device_decodable()                                    # the headers are intact: the plan takes it
    image, check = gb.decode_to_device("cuda:0")
    with pytest.raises(ValueError, match="block 5 "):
        check()
    tile_single_file(bad, str(tmp_path / "tiles"), buffer=0, tile_width=25, tile_height=25)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    with TD.Predictor(cfg, device_type="0", max_batch_size=4, output_dir=str(tmp_path / "out"), state_dict=sd) as pred:
        pred(bad, str(tmp_path / "tiles" / "bad.json"))
        assert pred.decode_stats["images"] == 0
    assert "using the host reader" in capsys.readouterr().out


def test_a_progressive_block_keeps_the_raster_on_the_host(tmp_path):
    import io
    from PIL import Image
    path = str(tmp_path / "p.tif")
    img = np.ascontiguousarray(make_tile(2, 64)[0].transpose(2, 0, 1))
    write_geotiff(path, img, T, 25832, compression="jpeg", tile=(32, 32))
    g = GeoTiff(path)
    g._setup_blocks()
    off, cnt = g._offs[1], g._counts[1]
    g.close()
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :32, 32:].transpose(1, 2, 0))).save(buf, "JPEG", quality=90, progressive=True)
    raw = bytearray(open(path, "rb").read())
    assert len(buf.getvalue()) <= cnt
    raw[off:off + len(buf.getvalue())] = buf.getvalue()
    open(path, "wb").write(bytes(raw))
    assert GeoTiff(path).device_decodable() is False


def test_prediction_files_are_identical_with_the_device_decoder_on_or_off(tmp_path):
    """A JPEG raster (tiles, 4:2:0) through the Predictor twice (the second time prefetched): windows cut in HBM from the device decode
    (device_decode auto) against the host reader (false) — byte-identical Prediction_*.json."""
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    rgb, _ = make_tile(300, 500)
    img = np.ascontiguousarray(rgb.transpose(2, 0, 1))
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    outs = {}
    for tag, dd in (("dev", "auto"), ("host", False)):
        d = tmp_path / tag
        (d / "rgb").mkdir(parents=True)
        tif = str(d / "rgb" / "9.tif")
        write_geotiff(tif, img, T, 25832, compression="jpeg", tile=(128, 128))
        tile_single_file(tif, str(d / "tiles"), buffer=10, tile_width=40, tile_height=40)
        with TD.Predictor(cfg, device_type="0", max_batch_size=3, output_dir=str(d / "out"), state_dict=sd, device_decode=dd) as pred:
            for _ in range(2):
                pred.prefetch(tif)
                pred(tif, str(d / "tiles" / "9.json"))
            assert pred.decode_stats["images"] == (2 if tag == "dev" else 0), (tag, pred.decode_stats)
        files = sorted(os.listdir(d / "out" / "9"))
        outs[tag] = {f: open(d / "out" / "9" / f, "rb").read().replace(tif.encode(), b"IMG") for f in files}
        assert len(files) == 9
    assert outs["dev"] == outs["host"]
    assert sum(len(json.loads(v)) for v in outs["dev"].values()) > 0
