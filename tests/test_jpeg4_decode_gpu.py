"""Four-band (RGBI) JPEG-in-TIFF rasters decoded on the GPU (jpegdecode.hip, mode 4: four components stored as they decode, one dword
per pixel) against the host reader (Pillow's libjpeg block by block): the same bytes for the writer's and libtiff's layouts, a corrupt
block reported by name with both consumers falling back, the crown stage's NDVI from the device-decoded raster, and the Predictor's
files unchanged with the device decoder on or off."""
import json
import os

import numpy as np
import pytest

from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


def _rgbi(h, w, seed=0):
    """[4, h, w]: synthetic orthophoto bands + a fourth band of its own (the green band mirrored, with a ramp and a flat area)."""
    rgb, _ = make_tile(seed, max(h, w))
    img = np.ascontiguousarray(np.concatenate([rgb[:h, :w], rgb[:h, :w, 1:2][:, ::-1]], axis=2).transpose(2, 0, 1))
    img[3, h // 5: h // 2, w // 8: w // 2] = 200
    img[:, -20:, -60:] = np.arange(60, dtype=np.uint8) * 4
    return img


def _device_equals_host(path, segments=None):
    g = GeoTiff(path)
    assert g.count == 4 and g.device_decodable()
    image, check = g.decode_to_device("cuda:0")
    got = check().cpu().numpy()
    ref = GeoTiff(path).read()
    assert got.shape == (g.height, g.width, 4)
    assert np.array_equal(got.transpose(2, 0, 1), ref), int((got.transpose(2, 0, 1) != ref).sum())
    assert check.compressed_bytes > 0 and check.kernel_ms > 0
    if segments is not None:
        assert check.segments == segments
    g.close()
    return got


@pytest.mark.parametrize("h,w,kw,segments", [(150, 200, {"tile": (64, 64)}, 12), (70, 100, {"rows_per_strip": 16}, 5),
                                             (128, 128, {"tile": (128, 128), "jpeg_restart": 1, "jpeg_tables": True}, 256)])
def test_device_decode_equals_the_host_reader(tmp_path, h, w, kw, segments):
    """A 3 x 4 grid of tiles cropped at the right and at the bottom; 100-wide strips of 16 rows with a 6-row last strip (a width that
    is no multiple of 8); one block of 256 one-MCU segments (more than one wave of lanes), tables in the JPEGTables tag."""
    path = str(tmp_path / "r.tif")
    write_geotiff(path, _rgbi(h, w, seed=h), T, 25832, compression="jpeg", **kw)
    got = _device_equals_host(path, segments)
    assert len(np.unique(got[:, :, 3])) > 20 and not np.array_equal(got[:, :, 3], got[:, :, 1])


@pytest.mark.parametrize("mode", ["RGBA", "CMYK", "RGBX"])
def test_device_decode_of_files_written_by_libtiff(tmp_path, mode):
    from PIL import Image
    a = np.ascontiguousarray(_rgbi(107, 128, seed=4).transpose(1, 2, 0))
    path = str(tmp_path / f"{mode}.tif")
    Image.fromarray(a, mode).save(path, compression="jpeg", quality=85, tiffinfo={278: 32})          # strips of 32 rows, the last one of 11
    assert GeoTiff(path).compression == 7
    _device_equals_host(path, 4)


def _corrupt(tmp_path, block):
    """A 200 x 200 RGBI raster of 64 x 64 tiles and a copy whose block ``block`` has 16 bytes of all-ones bits in the middle of its
    entropy-coded data (no code of the tables): the headers are intact, the plan takes it."""
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, _rgbi(200, 200, seed=9), T, 25832, compression="jpeg", tile=(64, 64))
    g = GeoTiff(good)
    g._setup_blocks()
    raw = bytearray(open(good, "rb").read())
    off, cnt = g._offs[block], g._counts[block]
    g.close()
    sos = raw.index(b"\xff\xda", off)
    mid = sos + (off + cnt - sos) // 2
    raw[mid:mid + 16] = b"\xff\x00" * 8
    open(bad, "wb").write(bytes(raw))
    return good, bad


def test_a_corrupt_block_is_reported_and_both_consumers_fall_back(tmp_path, capsys):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    good, bad = _corrupt(tmp_path, 5)
    gb = GeoTiff(bad)
    assert gb.device_decodable()
    image, check = gb.decode_to_device("cuda:0")
    with pytest.raises(ValueError, match="block 5 "):
        check()
    gb.close()
    capsys.readouterr()
    assert P._ndvi_on_device(GeoTiff(bad), 0.2, {"device_decode": True}, 0) is None
    log = capsys.readouterr().out
    assert f"device decode of {bad} failed" in log and "block 5 " in log and "using the host reader" in log
    assert P._ndvi_on_device(GeoTiff(good), 0.2, {"device_decode": True}, 0) is not None
    tile_single_file(bad, str(tmp_path / "tiles"), buffer=0, tile_width=20, tile_height=20)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    with TD.Predictor(cfg, device_type="0", max_batch_size=4, output_dir=str(tmp_path / "out"), state_dict=sd) as pred:
        pred(bad, str(tmp_path / "tiles" / "bad.json"))
        assert pred.decode_stats["images"] == 0
    assert "using the host reader" in capsys.readouterr().out


SIDE = 200                                                  # RGBI pixels of 0.2 m; the nDSM has SIDE / 5 pixels of 1 m
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318100.0)


def _scene(seed=21, crowns=6):
    """test_postprocessing_device_gpu's scene at 200 x 200: blob crowns, bright or dark in the near-infrared band, and their nDSM."""
    rng = np.random.default_rng(seed)
    rgbi = rng.integers(40, 120, (4, SIDE, SIDE), dtype=np.uint8)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    fine = rng.uniform(0, 1.0, (SIDE, SIDE)).astype(np.float32)
    rings = []
    for k in range(crowns):
        cx, cy, r = 35 + 65 * (k % 3) + rng.uniform(-5, 5), 50 + 100 * (k // 3) + rng.uniform(-5, 5), rng.uniform(14, 24)
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        inside = d2 < r ** 2
        rgbi[3][inside] = 220 if k % 3 else 60
        hgt = float(rng.uniform(1.2, 2.2) if k == 4 else rng.uniform(5.0, 25.0))
        fine[inside] = np.maximum(fine[inside], hgt * (1 - d2[inside] / r ** 2 * 0.5))
        ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        ring = np.stack([T[2] + T[0] * (cx + r * np.cos(ang)), T[5] + T[4] * (cy + r * np.sin(ang))], axis=1)
        rings.append(np.concatenate([ring, ring[:1]]))
    ndsm = fine.reshape(SIDE // 5, 5, SIDE // 5, 5).max(axis=(1, 3)).astype(np.float32)
    return rgbi, ndsm, rings, [0.97 - 0.015 * k for k in range(crowns)]


def _config(device_decode, n_scale):
    return {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 3.0,
            "ndvi_mean_threshold": 0.2, "ndvi_var_threshold": 0.5, "use_overlap": False, "tile_width": 50, "tile_height": 50,
            "buffer": 10, "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": n_scale,
            "height_scaling_factor": 1.0, "device_decode": device_decode}


@pytest.mark.parametrize("n_scale", [0.2, 1.0])
def test_crown_stage_takes_the_ndvi_from_the_device_decoded_raster(tmp_path, monkeypatch, n_scale):
    import torch
    rgbi, ndsm, rings, scores = _scene()
    rpath, hpath = str(tmp_path / "rgbi.tif"), str(tmp_path / "ndsm.tif")
    write_geotiff(rpath, rgbi, T, 25832, compression="jpeg", tile=(64, 64), jpeg_tables=True, jpeg_restart=4)
    write_geotiff(hpath, ndsm[None], NT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    rg = GeoTiff(rpath)
    ndvi = P._ndvi_on_device(rg, n_scale, _config(True, n_scale), 0)
    out = int(SIDE * n_scale)
    assert isinstance(ndvi, torch.Tensor) and ndvi.is_cuda and ndvi.dtype == torch.float32 and tuple(ndvi.shape) == (out, out)
    assert P._ndvi_on_device(rg, n_scale, _config("auto", n_scale), 0) is None and P._ndvi_on_device(rg, n_scale, _config(False, n_scale), 0) is None
    host = torch.from_numpy(np.ascontiguousarray(GeoTiff(rpath).read().transpose(1, 2, 0))).cuda()       # the host-decoded raster, uploaded as is
    ref = P.resample_on_device(host, out, out, [0, 3], "ndvi")
    assert torch.equal(ndvi.view(torch.int32), ref.view(torch.int32))
    assert float(ndvi.max()) > 0.3 and float(ndvi.min()) < 0
    rg.close()
    feats_host = P.process_layer(rings, scores, _config(False, n_scale), hpath, rpath)

    def no_host_reader(self):
        raise AssertionError(f"{self.path} went through the host reader")
    with monkeypatch.context() as m:
        m.setattr(GeoTiff, "read", no_host_reader)
        feats_dev = P.process_layer(rings, scores, _config(True, n_scale), hpath, rpath)
    assert 1 <= len(feats_host) < len(rings) and len(feats_dev) == len(feats_host)
    for fa, fb in zip(feats_host, feats_dev):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


def test_prediction_files_are_identical_with_the_device_decoder_on_or_off(tmp_path):
    """A four-band JPEG raster (tiles) through the Predictor twice (the second time prefetched): windows cut in HBM from the device
    decode, bands (2, 1, 0) of four (device_decode auto), against the host reader (false) — byte-identical Prediction_*.json."""
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    rgb, _ = make_tile(300, 500)
    img = np.ascontiguousarray(np.concatenate([rgb, 255 - rgb[:, :, :1]], axis=2).transpose(2, 0, 1))
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
