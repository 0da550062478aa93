"""Float32 height rasters decoded on the GPU (tiffdecode.hip: tiff_fp_blocks_to_image_kernel for predictor 3, the uint32 instance of
tiff_blocks_to_image_kernel for predictors 1 and 2) and handed to td_crown_stats where they lie: GeoTiff.decode_to_device against the
host reader and the source, bit for bit; rows wider than one step of the kernel; edge tiles through the raw entry point with guarded
memory around the raster; a corrupt block; crown_stats on the device tensor; process_layer with the device path on and off."""
import zlib

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff

from f32_cases import LAYOUTS, T, bits, fp_encode, height_raster, to_big_endian, write_float64

pytestmark = pytest.mark.gpu
H, W = 517, 683


def _decode(path):
    g = GeoTiff(path)
    image, check = g.decode_to_device("cuda:0")
    out = check()
    assert check.kernel_ms > 0 and check.compressed_bytes > 0
    return g, out


@pytest.mark.parametrize("bands", [1, 3, 4])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("predictor", [1, 2, 3])
@pytest.mark.parametrize("codec", ["lzw", "deflate"])
def test_device_decode_equals_the_host_reader_and_the_source(tmp_path, codec, predictor, layout, bands):
    img = height_raster(bands, H, W, seed=10 * predictor + bands)
    path = str(tmp_path / "f.tif")
    write_geotiff(path, img, T, 25832, compression=codec, predictor=predictor, **LAYOUTS[layout])
    g = GeoTiff(path)
    assert not g.device_decodable() and g.device_decodable(float_samples=True)
    g, out = _decode(path)
    assert out.dtype == torch.float32 and tuple(out.shape) == (H, W, bands) and out.is_cuda
    got = out.cpu().numpy().transpose(2, 0, 1)
    assert np.array_equal(bits(got), bits(img))
    assert np.array_equal(bits(got), bits(GeoTiff(path).read()))


def test_rows_wider_than_one_step_carry_across_steps(tmp_path):
    """3 x 70 001 px, one strip per row, predictor 3: 274 steps of 256 positions per plane with carries between them, planes that begin
    at odd bytes (70 001 is odd), a last step of 113 positions."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 1 << 32, (1, 3, 70001), dtype=np.uint64).astype(np.uint32).view(np.float32)
    img[0, 1] = np.linspace(0, 30, 70001, dtype=np.float32)
    for codec in ("deflate", "lzw"):
        path = str(tmp_path / f"wide_{codec}.tif")
        write_geotiff(path, img, T, 25832, compression=codec, predictor=3, rows_per_strip=1)
        g, out = _decode(path)
        assert np.array_equal(bits(out.cpu().numpy()[:, :, 0]), bits(img[0])), codec


SENTINEL = 0xDEADBEEF
GUARD = 1 << 16


@pytest.mark.parametrize("spp", [1, 2, 3, 4])
@pytest.mark.parametrize("predictor", [1, 2, 3])
def test_edge_tiles_write_only_inside_the_raster(spp, predictor):
    """256 x 256 tiles on a 300 x 300 raster through td_tiff_blocks_to_image_f32_dev itself: the raster lies in the middle of a buffer
    filled with a sentinel; the 64 Ki floats before and after it still hold the sentinel afterwards, the raster holds the source."""
    lib = _lib.load()
    h = w = 300
    bh = bw = 256
    rng = np.random.default_rng(spp + 10 * predictor)
    src = rng.integers(0, 1 << 32, (h, w, spp), dtype=np.uint64).astype(np.uint32)
    blocks = np.zeros((2, 2, bh, bw * spp * 4), np.uint8)
    for by in range(2):
        for bx in range(2):
            tile = rng.integers(0, 1 << 32, (bh, bw, spp), dtype=np.uint64).astype(np.uint32)      # (the padding is not zero: it takes part in the sums)
            piece = src[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
            tile[:piece.shape[0], :piece.shape[1]] = piece
            if predictor == 3:
                enc = fp_encode(tile.view(np.float32))
            elif predictor == 2:
                d = tile.copy()
                d[:, 1:] = tile[:, 1:] - tile[:, :-1]
                enc = d.reshape(bh, -1).view(np.uint8)
            else:
                enc = tile.reshape(bh, -1).view(np.uint8)
            blocks[by, bx] = enc
    d_blocks = torch.from_numpy(blocks.reshape(4, -1)).cuda()
    cap = d_blocks.shape[1]
    n = h * w * spp
    buf = torch.full((GUARD + n + GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    image = buf[GUARD:GUARD + n]
    st = lib.td_tiff_blocks_to_image_f32_dev(d_blocks.data_ptr(), cap, bw, bh, 2, 2, spp, predictor, image.data_ptr(), w, h, _lib.stream_ptr())
    _lib.check(st, "td_tiff_blocks_to_image_f32_dev")
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all()
    assert np.array_equal(got[GUARD:GUARD + n].reshape(h, w, spp), src)


def test_the_entry_point_checks_its_arguments_as_the_integer_forms_do():
    lib = _lib.load()
    blocks = torch.zeros((4, 64 * 64 * 4), dtype=torch.uint8, device="cuda")
    image = torch.zeros((100 * 100,), dtype=torch.float32, device="cuda")
    sp = _lib.stream_ptr()
    ok = (blocks.data_ptr(), blocks.shape[1], 64, 64, 2, 2, 1, 3, image.data_ptr(), 100, 100, sp)
    assert lib.td_tiff_blocks_to_image_f32_dev(*ok) == 0
    for k, v in ((0, None), (8, None), (7, 0), (7, 4), (6, 0), (6, 5), (4, 1), (5, 3), (1, 64 * 64 * 4 - 4), (1, 64 * 64 * 4 + 2), (2, 0), (9, 0)):
        bad = list(ok)
        bad[k] = v
        assert lib.td_tiff_blocks_to_image_f32_dev(*bad) == _lib.ERR_INVALID, (k, v)
    u8 = torch.zeros((100 * 100,), dtype=torch.uint8, device="cuda")
    assert lib.td_tiff_blocks_to_image_dev(blocks.data_ptr(), blocks.shape[1], 64, 64, 2, 2, 1, 3, u8.data_ptr(), 100, 100, sp) == _lib.ERR_INVALID
    torch.cuda.synchronize()


# ---- the consumer --------------------------------------------------------------------------------------------------------
def _scene(tmp_path, seed=9):
    """An RGBI image (0.2 m, 300 x 300) and an nDSM on a 1 m grid (60 x 60) with blob crowns of known height, plus their rings."""
    rng = np.random.default_rng(seed)
    side = 300
    t = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318060.0)
    rgbi = rng.integers(40, 120, (4, side, side), dtype=np.uint8)
    yy, xx = np.mgrid[0:side, 0:side]
    fine = rng.uniform(0, 1.0, (side, side)).astype(np.float32)
    crowns = []
    for k in range(14):
        cx, cy, r = rng.uniform(30, 270), rng.uniform(30, 270), rng.uniform(8, 25)
        inside = (xx - cx) ** 2 + (yy - cy) ** 2 < r ** 2
        rgbi[3][inside] = 220 if k % 4 else 60
        hgt = float(rng.uniform(1.0, 25.0))
        fine[inside] = np.maximum(fine[inside], hgt * (1 - ((xx - cx) ** 2 + (yy - cy) ** 2)[inside] / r ** 2 * 0.5))
        ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        ring = np.stack([t[2] + t[0] * (cx + r * np.cos(ang)), t[5] + t[4] * (cy + r * np.sin(ang))], axis=1)
        crowns.append(np.concatenate([ring, ring[:1]]))
    ndsm = fine.reshape(60, 5, 60, 5).max(axis=(1, 3)).astype(np.float32)
    nt = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318060.0)
    rgbi_path = str(tmp_path / "rgbi.tif")
    write_geotiff(rgbi_path, rgbi, t, 25832)
    scores = [0.95 - 0.03 * k for k in range(len(crowns))]
    return rgbi_path, ndsm, nt, crowns, scores


def _config(device_decode, h_scale=1.0):
    return {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 3,
            "ndvi_mean_threshold": 0.2, "ndvi_var_threshold": 0.5, "use_overlap": False, "tile_width": 50, "tile_height": 50, "buffer": 10,
            "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": 1.0, "height_scaling_factor": h_scale,
            "device_decode": device_decode}


def _outcome(fn):
    try:
        return ("features", fn())
    except Exception as e:                                  # noqa: BLE001 — the outcome IS the exception when the host reader raises
        return ("raised", type(e).__name__, str(e))


def _same_features(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


@pytest.fixture
def height_loads(monkeypatch):
    """Counts GeoTiff._load calls per path (a whole-raster read on the host)."""
    calls = {}
    real = GeoTiff._load

    def counted(self):
        calls[self.path] = calls.get(self.path, 0) + 1
        return real(self)
    monkeypatch.setattr(GeoTiff, "_load", counted)
    return calls


def test_process_layer_is_identical_with_the_height_raster_decoded_on_the_device(tmp_path, height_loads):
    rgbi_path, ndsm, nt, crowns, scores = _scene(tmp_path)
    hpath = str(tmp_path / "ndsm.tif")
    write_geotiff(hpath, ndsm[None], nt, 25832, compression="deflate", predictor=3, tile=(32, 32))
    assert GeoTiff(hpath).device_decodable(float_samples=True)
    host = P.process_layer(crowns, scores, _config(False), hpath, rgbi_path)
    assert height_loads.get(hpath) == 1
    dev = P.process_layer(crowns, scores, _config(True), hpath, rgbi_path)
    assert height_loads.get(hpath) == 1                     # the second run did not read the height raster on the host
    assert len(host) >= 3 and any(f["properties"]["TreeHeight"] > 3 for f in host)
    _same_features(host, dev)
    cfg = _config("auto")                                   # "auto", the key's default, keeps the host reader for the height raster
    _same_features(host, P.process_layer(crowns, scores, cfg, hpath, rgbi_path))
    del cfg["device_decode"]
    _same_features(host, P.process_layer(crowns, scores, cfg, hpath, rgbi_path))
    assert height_loads.get(hpath) == 3


@pytest.mark.parametrize("mode", [0, 1])
def test_crown_stats_reads_a_device_tensor_where_it_lies(tmp_path, mode):
    rgbi_path, ndsm, nt, crowns, _ = _scene(tmp_path, seed=4)
    ndsm = ndsm.copy()
    ndsm[7, 9], ndsm[30, 31] = np.float32(-0.0), np.float32(1e-40)
    hpath = str(tmp_path / "ndsm.tif")
    write_geotiff(hpath, ndsm[None], nt, 25832, compression="lzw", predictor=3, rows_per_strip=7)
    g, out = _decode(hpath)
    tensor = out.view(g.height, g.width)
    ptr = tensor.data_ptr()
    circles = P.crown_circles(crowns)
    hb = (nt[2], nt[5] + nt[4] * ndsm.shape[0], nt[2] + nt[0] * ndsm.shape[1], nt[5])
    from_host = P.crown_stats(ndsm, nt, hb, circles, mode)
    from_dev = P.crown_stats(tensor, nt, hb, circles, mode)
    assert tensor.data_ptr() == ptr and from_dev.shape == (len(crowns), 3 if mode == 0 else 4)
    assert np.array_equal(bits(from_dev), bits(from_host))
    assert np.array_equal(bits(P.crown_stats(tensor, nt, hb, circles, mode, 0.5, clamp_shape=tensor.shape)),
                          bits(P.crown_stats(ndsm, nt, hb, circles, mode, 0.5, clamp_shape=ndsm.shape)))
    for bad in (tensor.cpu(), tensor.double(), tensor.t(), tensor[None]):
        with pytest.raises(ValueError, match="contiguous float32 CUDA tensor"):
            P.crown_stats(bad, nt, hb, circles, mode)


def test_a_corrupt_block_is_reported_and_the_host_reader_serves_the_image(tmp_path, capsys):
    """One bit of block 2's Adler-32 trailer flipped: check() names the block; process_layer prints that and takes the host path, whose
    outcome it returns — here zlib's own "incorrect data check" on the same block, exactly as with the device path off."""
    rgbi_path, ndsm, nt, crowns, scores = _scene(tmp_path)
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, ndsm[None], nt, 25832, compression="deflate", predictor=3, tile=(32, 32))
    g = GeoTiff(good)
    g._setup_blocks()
    off, cnt = int(g._offs[2]), int(g._counts[2])
    g.close()
    raw = bytearray(open(good, "rb").read())
    raw[off + cnt - 2] ^= 0x10
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(zlib.error, match="incorrect data check"):
        zlib.decompress(bytes(raw[off:off + cnt]))
    image, check = GeoTiff(bad).decode_to_device("cuda:0")
    with pytest.raises(ValueError, match="block 2: Adler-32 mismatch"):
        check()
    capsys.readouterr()
    host = _outcome(lambda: P.process_layer(crowns, scores, _config(False), bad, rgbi_path))
    assert "using the host reader" not in capsys.readouterr().out
    dev = _outcome(lambda: P.process_layer(crowns, scores, _config(True), bad, rgbi_path))
    log = capsys.readouterr().out
    assert "block 2: Adler-32 mismatch" in log and "using the host reader" in log
    assert host[0] == "raised" and "incorrect data check" in host[2] and dev == host
    # the untouched file: both paths, same features
    _same_features(P.process_layer(crowns, scores, _config(False), good, rgbi_path), P.process_layer(crowns, scores, _config(True), good, rgbi_path))


@pytest.mark.parametrize("case", ["big_endian", "planar", "float64", "scaled"])
def test_rasters_the_device_path_refuses_keep_the_host_path(tmp_path, height_loads, case):
    rgbi_path, ndsm, nt, crowns, scores = _scene(tmp_path)
    hpath = str(tmp_path / "ndsm.tif")
    h_scale = 1.0
    if case == "big_endian":
        le = str(tmp_path / "le.tif")
        write_geotiff(le, ndsm[None], nt, 25832, compression="deflate", predictor=3, tile=(32, 32))
        to_big_endian(le, hpath)
    elif case == "planar":
        write_geotiff(hpath, ndsm[None], nt, 25832, compression="deflate", predictor=3, tile=(32, 32), planar=True)
    elif case == "float64":
        write_float64(hpath, ndsm, nt, compression="deflate", rows_per_strip=8)
        assert GeoTiff(hpath).dtype == np.float64 and np.array_equal(GeoTiff(hpath).read()[0], ndsm.astype(np.float64))
    else:
        write_geotiff(hpath, ndsm[None], nt, 25832, compression="deflate", predictor=3, tile=(32, 32))
        h_scale = 2.0
    g = GeoTiff(hpath)
    assert bool(g.device_decodable(float_samples=True)) == (case == "scaled") and np.array_equal(g.read()[0].astype(np.float32), ndsm)
    height_loads.clear()
    host = P.process_layer(crowns, scores, _config(False, h_scale), hpath, rgbi_path)
    dev = P.process_layer(crowns, scores, _config(True, h_scale), hpath, rgbi_path)
    assert height_loads.get(hpath) == 2                     # both runs read it on the host
    assert len(host) >= 3
    _same_features(host, dev)
