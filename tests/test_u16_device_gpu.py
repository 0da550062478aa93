"""16-bit rasters kept on the GPU from decode to model input: the decoded / uploaded raster in HBM equals the host reader's samples
exactly; td_windows_u16_to_input (the rule of reference prediction.py:166-169 + the float resize, two launches) is bit-equal to the
host path — numpy BGR pick, 255 * x / 65535 in float64, td_resize_bilinear_f64 — padding included; prediction files are
byte-identical with the device path on or off; a corrupt block sends the image back to the host reader."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from gpu_util import dev
from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


def _raster16(bands, h, w, seed=0):
    """Imagery x 257 (0 .. 65535), a block of noise over the full range, a flat area and ramps whose differences wrap modulo 65536."""
    rgb, _ = make_tile(seed, max(h, w))
    img = (np.concatenate([rgb, rgb[..., 1:2]], axis=2)[:h, :w, :bands].astype(np.uint16) * 257).transpose(2, 0, 1).copy()
    rng = np.random.default_rng(seed)
    img[:, : h // 4, w // 2:] = rng.integers(0, 65536, (bands, h // 4, w - w // 2), dtype=np.uint16)
    img[:, h // 5: h // 2, w // 8: w // 2] = 0xfffe                                              # flat: long strings
    img[:, -40:, -90:] = (np.arange(90, dtype=np.uint32) * 4099 % 65536).astype(np.uint16)       # constant differences that wrap
    img[:, -41, :] = np.where(np.arange(w) % 2 == 0, 0, 65535).astype(np.uint16)                 # +65535 / -65535 steps
    return img


@pytest.mark.parametrize("codec", ["lzw", "deflate"])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("layout", [{"tile": (128, 128)}, {"tile": (64, 256)}, {"rows_per_strip": 7}, {"rows_per_strip": 1}])
@pytest.mark.parametrize("bands", [1, 3, 4])
def test_device_decode_of_uint16_equals_the_host_reader(tmp_path, codec, predictor, layout, bands):
    img = _raster16(bands, 517, 683, seed=bands)
    assert img.min() == 0 and img.max() == 65535
    path = str(tmp_path / "r.tif")
    write_geotiff(path, img, T, 25832, compression=codec, predictor=predictor, **layout)
    g = GeoTiff(path)
    assert g.device_decodable()
    image, check = g.decode_to_device("cuda:0")
    got = check().cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == (517, 683, bands)
    assert np.array_equal(got.transpose(2, 0, 1), GeoTiff(path).read())
    assert np.array_equal(got.transpose(2, 0, 1), img)


@pytest.mark.parametrize("kw", [{}, {"rows_per_strip": 16}])
def test_device_upload_of_uint16_equals_the_host_reader(tmp_path, kw):
    img = _raster16(3, 517, 683, seed=8)
    path = str(tmp_path / "r.tif")
    write_geotiff(path, img, T, 25832, **kw)
    g = GeoTiff(path)
    assert g.device_uploadable()
    image, check = g.upload_to_device("cuda:0", piece=1 << 16, staging=[torch.empty((1 << 18,), dtype=torch.uint8, pin_memory=True) for _ in range(2)])
    got = check().cpu().numpy()
    assert got.dtype == np.uint16 and np.array_equal(got.transpose(2, 0, 1), GeoTiff(path).read())
    assert check.compressed_bytes == img.nbytes


def _host_input(raster_hwc, win, oh, ow, rows, pitch):
    """One window as the host path feeds the engine: crop, rasterio.mask's zeros, BGR pick, the rule, float64 →
    td_resize_bilinear_f64 into a padded float32 buffer (prediction.py: _process_tile, Engine.preprocess_tiles_f64)."""
    r0, c0, h, w, vy0, vy1, vx0, vx1 = win
    hwc = raster_hwc[r0:r0 + h, c0:c0 + w].copy()
    keep = np.zeros((h, w), bool)
    keep[vy0:vy1, vx0:vx1] = True
    hwc[~keep] = 0
    out_img = hwc.transpose(2, 0, 1)
    bgr = np.stack((out_img[2], out_img[1], out_img[0])).astype(np.float64)
    flag = int(np.max(out_img[1]))
    if flag > 255:
        bgr = 255.0 * bgr / 65535.0
    dst = torch.full((3, rows, pitch), -1.0, dtype=torch.float32, device="cuda")
    d = dev(bgr)
    _lib.check(_lib.load().td_resize_bilinear_f64(d.data_ptr(), 3, h, w, dst.data_ptr(), oh, ow, pitch, rows * pitch, _lib.stream_ptr()),
               "td_resize_bilinear_f64")
    torch.cuda.synchronize()
    return dst.cpu().numpy(), bgr, flag


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("h,w,oh,ow", [(450, 450, 800, 800), (1000, 1000, 800, 800), (350, 450, 800, 1029), (97, 211, 613, 1333), (800, 800, 800, 800)])
def test_windows_u16_to_input_is_bit_equal_to_the_host_path(h, w, oh, ow, bands):
    """Three windows of one size in ONE call: band 1 above 255 (rule on), band 1 <= 255 with the other bands over the full range (rule
    off — the flag is per window), and a rule-on window of which rasterio.mask keeps an inner rectangle only. Bit-equal to the host
    path on the whole padded buffer; against F.interpolate in float64 on the CPU the bound of
    test_resize_bilinear_f64_matches_torch_interpolate holds (<= 1 float32 ulp everywhere, >= 0.9999 equal)."""
    import torch.nn.functional as F
    lib = _lib.load()
    rng = np.random.default_rng(h * 13 + w + bands)
    H, W = 2 * h + 37, w + 53
    raster = rng.integers(0, 65536, (H, W, bands), dtype=np.uint16)
    raster[h + 30:, :, 1] = rng.integers(0, 256, (H - h - 30, W), dtype=np.uint16)      # the lower part: band 1 stays <= 255
    raster[h + 30 + h // 2, 17 + w // 2, 1] = 255                                          # (the threshold itself is still "off")
    wins = np.array([[11, 29, h, w, 0, h, 0, w],
                     [h + 33, 17, h, w, 0, h, 0, w],
                     [5, 50, h, w, 3, h - 1, 2, w - 5]], dtype=np.int32)
    pitch, rows = (ow + 31) // 32 * 32, (oh + 31) // 32 * 32
    d_raster = dev(raster)
    assert d_raster.dtype == torch.uint16
    dst = torch.full((3, 3, rows, pitch), -1.0, dtype=torch.float32, device="cuda")
    flags = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.td_windows_u16_to_input(d_raster.data_ptr(), H, W, bands, wins.ctypes.data, 3, flags.data_ptr(), dst.data_ptr(), oh, ow, pitch,
                                           rows * pitch, 3 * rows * pitch, _lib.stream_ptr()), "td_windows_u16_to_input")
    torch.cuda.synchronize()
    got, got_flags = dst.cpu().numpy(), flags.cpu().numpy()
    rule = []
    for i, win in enumerate(wins):
        want, bgr, flag = _host_input(raster, win, oh, ow, rows, pitch)
        rule.append(flag > 255)
        assert got_flags[i] == flag, (i, got_flags[i], flag)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, int((got[i] != want).sum()))
        ref = F.interpolate(torch.from_numpy(bgr)[None], size=(oh, ow), mode="bilinear", align_corners=False)[0].float().numpy()
        out = got[i][:, :oh, :ow]
        ulp = np.spacing(np.abs(ref).astype(np.float32))
        print(f"window {i}: max |got - ref| / ulp = {float((np.abs(out - ref) / ulp).max()):.3f}, equal {float((out == ref).mean()):.6f}")
        assert (np.abs(out - ref) <= ulp).all()
        assert (out == ref).mean() >= 0.9999
        assert (got[i][:, oh:, :] == -1.0).all() and (got[i][:, :, ow:] == -1.0).all()      # nothing written outside the image
    assert rule == [True, False, True]


def test_windows_u16_to_input_refuses_windows_outside_the_raster():
    lib = _lib.load()
    d_raster = dev(np.zeros((40, 50, 3), np.uint16))
    dst = torch.zeros((1, 3, 32, 32), dtype=torch.float32, device="cuda")
    flags = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for win in ([30, 0, 20, 20, 0, 20, 0, 20], [0, 40, 20, 20, 0, 20, 0, 20], [-1, 0, 20, 20, 0, 20, 0, 20], [0, 0, 20, 20, 0, 21, 0, 20]):
        w = np.array([win], dtype=np.int32)
        st = lib.td_windows_u16_to_input(d_raster.data_ptr(), 40, 50, 3, w.ctypes.data, 1, flags.data_ptr(), dst.data_ptr(), 32, 32, 32, 32 * 32,
                                         3 * 32 * 32, _lib.stream_ptr())
        assert st < 0, win


def _sixteen_bit_scene():
    """500 x 500 x 3 uint16: imagery x 257 on the right (band 1 far above 255: the rule rescales those tiles), the same imagery as it
    is (<= 255) in the left 260 columns (tiles that lie there stay unscaled)."""
    rgb, _ = make_tile(300, 500)
    img = np.ascontiguousarray((rgb.astype(np.uint16) * 257).transpose(2, 0, 1))
    img[:, :, :260] = rgb.transpose(2, 0, 1)[:, :, :260]
    return img


def test_prediction_files_are_identical_with_the_16_bit_device_path_on_or_off(tmp_path):
    """A uint16 LZW raster (tiles, predictor 2) over two images with the host reader (device_decode False) and decoded into HBM
    ("auto"), and the same samples stored uncompressed and uploaded whole ("all"): byte-identical Prediction_*.json. One tile's
    bounds lie off the pixel grid (rasterio.mask's centre rule → a valid rectangle inside the window)."""
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    img = _sixteen_bit_scene()
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    lzw = {"compression": "lzw", "tile": (128, 128), "predictor": 2}
    outs = {}
    for tag, kw, dd in (("lzw_host", lzw, False), ("lzw_dev", lzw, "auto"), ("raw_dev", {}, "all")):
        d = tmp_path / tag
        (d / "rgb").mkdir(parents=True)
        tif = str(d / "rgb" / "9.tif")
        write_geotiff(tif, img, T, 25832, **kw)
        tile_single_file(tif, str(d / "tiles"), buffer=10, tile_width=40, tile_height=40)
        meta = json.load(open(d / "tiles" / "9.json"))
        k0 = next(iter(meta))
        b = meta[k0]["bounds"]
        meta[k0]["bounds"] = [b[0] + 0.1, b[1] + 0.1, b[2] - 0.1, b[3] - 0.1] + list(b[4:])      # half a pixel inwards on every side
        json.dump(meta, open(d / "tiles" / "9.json", "w"))
        g = GeoTiff(tif)
        over = []
        for t in meta.values():
            c0, r0, w, h = g.window_of_bounds(t["bounds"][:4])
            over.append(int(img[1, r0:r0 + h, c0:c0 + w].max()) > 255)
        assert any(over) and not all(over)                        # tiles on both sides of the rule
        with TD.Predictor(cfg, device_type="0", max_batch_size=3, output_dir=str(d / "out"), state_dict=sd, device_decode=dd) as pred:
            for _ in range(2):                                      # twice: the second image is prefetched by the first's walk
                pred.prefetch(tif)
                pred(tif, str(d / "tiles" / "9.json"))
            assert pred.decode_stats["images"] == (2 if tag == "lzw_dev" else 0), (tag, pred.decode_stats)
            assert pred.upload_stats["images"] == (2 if tag == "raw_dev" else 0), (tag, pred.upload_stats)
            if tag != "lzw_host":
                st = pred.decode_stats if tag == "lzw_dev" else pred.upload_stats
                assert st["decoded_bytes"] == 2 * img.nbytes, st      # bytes, not samples
        files = sorted(os.listdir(d / "out" / "9"))
        outs[tag] = {f: open(d / "out" / "9" / f, "rb").read().replace(tif.encode(), b"IMG") for f in files}
        assert len(files) == 9
    assert outs["lzw_host"] == outs["lzw_dev"] == outs["raw_dev"]
    assert sum(len(json.loads(v)) for v in outs["lzw_host"].values()) > 0


def test_a_truncated_uint16_block_is_reported_and_the_predictor_falls_back(tmp_path, capsys):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    img = _sixteen_bit_scene()
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, img, T, 25832, compression="lzw", tile=(128, 128))
    g = GeoTiff(good)
    g._setup_blocks()
    raw = bytearray(open(good, "rb").read())
    counts = struct.pack(f"<{len(g._counts)}I", *g._counts)
    at = raw.find(counts)
    assert at > 0 and raw.find(counts, at + 1) < 0
    struct.pack_into("<I", raw, at + 4 * 5, g._counts[5] // 2)       # block 5 ends half way: it decodes to fewer bytes than a tile holds
    open(bad, "wb").write(bytes(raw))
    assert GeoTiff(bad).device_decodable()
    image, check = GeoTiff(bad).decode_to_device("cuda:0")
    with pytest.raises(ValueError, match="block 5"):
        check()
    # the Predictor logs it and serves the image through the host reader — whose decoder rejects the same block: the tiles that
    # need it are dropped (reference prediction.py:174-176), the others are predicted
    tile_single_file(bad, str(tmp_path / "tiles"), buffer=0, tile_width=25, tile_height=25)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    with TD.Predictor(cfg, device_type="0", max_batch_size=4, output_dir=str(tmp_path / "out"), state_dict=sd) as pred:
        pred(bad, str(tmp_path / "tiles" / "bad.json"))
        assert pred.decode_stats["images"] == 0
    assert "using the host reader" in capsys.readouterr().out
    files = os.listdir(tmp_path / "out" / "bad")
    assert 0 < len(files) < 16
