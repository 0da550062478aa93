"""Band-separate (PlanarConfiguration = 2) GeoTIFFs decoded on the GPU (``device_decode_planar``; tiffdecode.hip:
td_tiff_planes_to_image_dev / _u16_dev / _f32_dev after the unchanged block decoders). The layout kernels alone against numpy on random
blocks, byte for byte; files of every codec, sample type, predictor, band count and block layout against the source array and the host
reader; plane subsets; more blocks than decoder waves; a damaged block; the Predictor's files and the crown stage's features with the
key on and off."""
import json
import os

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import device_decode as D
from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)
ENTRY = {1: "td_tiff_planes_to_image_dev", 2: "td_tiff_planes_to_image_u16_dev", 4: "td_tiff_planes_to_image_f32_dev"}
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)     # the dword edge, the wave edge, the 256-pixel step, a carry across steps
GUARD = 4096


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------------
def _planes_oracle(blocks, item, bw, bh, nx, ny, spp, mask, predictor, width, height):
    """numpy: every selected band's blocks → [height, width, spp] of DTYPE[item]; cumulative sums modulo the sample width for predictor
    2, td_tiff_unpredict_float for predictor 3; channels that are not selected are 0."""
    out = np.zeros((height, width, spp), dtype=DTYPE[item])
    slot = 0
    for c in range(spp):
        if not (mask >> c) & 1:
            continue
        for by in range(ny):
            for bx in range(nx):
                raw = np.array(blocks[(slot * ny + by) * nx + bx, :bw * bh * item])
                if predictor == 3:
                    _lib.check(_lib.load().td_tiff_unpredict_float(raw.ctypes.data, bh, bw, 1, 4), "td_tiff_unpredict_float")
                blk = raw.view(DTYPE[item]).reshape(bh, bw)
                if predictor == 2:
                    blk = np.cumsum(blk, axis=1, dtype=DTYPE[item])
                y0, x0 = by * bh, bx * bw
                rows, cols = min(bh, height - y0), min(bw, width - x0)
                out[y0:y0 + rows, x0:x0 + cols, c] = blk[:rows, :cols]
        slot += 1
    return out


def _run_planes(rng, item, spp, mask, bw, bh, pad, keep, predictor, shift=0):
    """One launch on random blocks; → (got, want) as byte arrays. ``keep``: pixels of the last block column inside the raster; ``pad``:
    bytes of capacity behind a block; ``shift``: bytes by which the block buffer is moved off its alignment. The image lies between
    guards, everything filled with 0xFF beforehand."""
    nx, ny = (3 if bw < 300 else 2), 2
    width, height = (nx - 1) * bw + keep, (ny - 1) * bh + (bh + 1) // 2
    cap = bw * bh * item + pad
    nsel = bin(mask).count("1")
    blocks = rng.integers(0, 256, (nsel * nx * ny, cap), dtype=np.uint8)
    d_buf = torch.empty((blocks.size + 16,), dtype=torch.uint8, device="cuda")
    d_blocks = d_buf[shift:shift + blocks.size]
    d_blocks.copy_(torch.from_numpy(blocks.reshape(-1)))
    nbytes = width * height * spp * item
    d_image = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    st = getattr(_lib.load(), ENTRY[item])(d_blocks.data_ptr(), cap, bw, bh, nx, ny, spp, mask, predictor, d_image.data_ptr() + GUARD, width, height,
                                           _lib.stream_ptr())
    _lib.check(st, ENTRY[item])
    got = d_image.cpu().numpy()
    assert (got[:GUARD] == 0xFF).all() and (got[GUARD + nbytes:] == 0xFF).all(), "a store outside the image"
    want = _planes_oracle(blocks, item, bw, bh, nx, ny, spp, mask, predictor, width, height)
    return got[GUARD:GUARD + nbytes], want.reshape(-1).view(np.uint8)


KERNEL_CASES = [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3)]
PADS = {1: (0, 3, 8), 2: (0, 6), 4: (0, 12)}               # exact, padded; uint8 / uint16: a capacity that is no multiple of 4


@pytest.mark.parametrize("item,predictor", KERNEL_CASES)
def test_the_layout_kernels_equal_numpy_at_every_block_width(item, predictor):
    rng = np.random.default_rng(100 * item + predictor)
    combos = [(4, 0b1111), (3, 0b111), (2, 0b11), (1, 1), (4, 0b1001), (3, 0b101)]
    k = 0
    for bw in WIDTHS:
        for bh in (1, 3):
            for pad in PADS[item]:
                for keep in (1, bw):
                    spp, mask = combos[k % len(combos)]
                    k += 1
                    got, want = _run_planes(rng, item, spp, mask, bw, bh, pad, keep, predictor)
                    assert np.array_equal(got, want), (item, predictor, bw, bh, pad, keep, spp, bin(mask))
    # four bands, every width, exact capacity: the whole-pixel stores (uint8: when the rows are dwords, and when they are not)
    for bw in WIDTHS:
        got, want = _run_planes(rng, item, 4, 0b1111, bw, 3, 0, bw, predictor)
        assert np.array_equal(got, want), (item, predictor, bw)


@pytest.mark.parametrize("item,predictor", KERNEL_CASES)
def test_every_plane_mask_and_zeros_for_the_planes_left_out(item, predictor):
    """The image is 0xFF before the launch: a channel whose plane was not selected must come out 0, not stay."""
    rng = np.random.default_rng(200 * item + predictor)
    for spp in (1, 2, 3, 4):
        for mask in range(1, 1 << spp):
            for bw, keep in ((5, 1), (64, 64), (257, 257)):
                got, want = _run_planes(rng, item, spp, mask, bw, 3, 0, keep, predictor)
                assert np.array_equal(got, want), (item, predictor, spp, bin(mask), bw)
                px = got.view(DTYPE[item]).reshape(-1, spp)
                for c in range(spp):
                    if not (mask >> c) & 1:
                        assert not px[:, c].any(), (spp, bin(mask), c)


def test_block_buffers_off_their_alignment_take_the_sample_wise_path():
    """uint8 blocks may begin at any byte: the same pixels as from an aligned buffer."""
    rng = np.random.default_rng(7)
    for shift in (1, 2, 3):
        for bw in (4, 64, 256):
            for spp, mask in ((4, 0b1111), (4, 0b1001), (3, 0b111), (1, 1)):
                got, want = _run_planes(rng, 1, spp, mask, bw, 3, 0, bw, 2, shift=shift)
                assert np.array_equal(got, want), (shift, bw, spp, bin(mask))


# ---- 2. files ------------------------------------------------------------------------------------------------------------------------
def _raster(bands, h, w, dtype, seed=0):
    """Texture with a flat area (long matches) and ramps (constant differences under predictor 2); uint16 fills both bytes, float32 has
    fractions and negative values."""
    rgb, _ = make_tile(seed, max(h, w, 64))
    reps = (-(-h // rgb.shape[0]), -(-w // rgb.shape[1]), 1)
    img = np.tile(np.concatenate([rgb, rgb[..., 1:2]], axis=2), reps)[:h, :w, :bands].transpose(2, 0, 1).astype(np.int64)
    img[:, h // 5: h // 2, w // 8: w // 2] = 7
    img[:, -min(40, h):, -min(90, w):] = np.arange(min(90, w))
    if dtype == np.uint8:
        return img.astype(np.uint8)
    if dtype == np.uint16:
        return ((img * 257 + np.arange(w)[None, None, :] * 3) % 65536).astype(np.uint16)
    return (img.astype(np.float32) * np.float32(0.37) - np.float32(31.25)).astype(np.float32)


def _write(path, img, transform=T, **kw):
    try:
        write_geotiff(path, img, transform, 25832, planar=True, **kw)
    except ValueError as e:
        if kw.get("compression") == "zstd" and "libzstd" in str(e):
            pytest.skip(str(e))
        raise


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _decode(path, **kw):
    g = GeoTiff(path)
    assert g.planar == 2 and not g.device_decodable(float_samples=True) and g.device_decodable(float_samples=True, planar=True)
    image, check = g.decode_to_device("cuda:0", planar=True, **kw)
    return check().cpu().numpy(), check


LAYOUTS = [{"tile": (16, 16)}, {"tile": (64, 256)}, {"tile": (128, 128)}, {"rows_per_strip": 1}, {"rows_per_strip": 7}, {"rows_per_strip": 157}]
SAMPLES = [(np.uint8, 1), (np.uint8, 2), (np.uint16, 1), (np.uint16, 2), (np.float32, 1), (np.float32, 2), (np.float32, 3)]
# every sample type and predictor in every layout; the codec and the band count rotate so that each codec meets each sample type and
# predictor, each layout and each band count
FILE_CASES = [(("lzw", "deflate", "zstd")[(i + j) % 3], SAMPLES[i], 1 + (i + j) % 4, LAYOUTS[j]) for i in range(len(SAMPLES)) for j in range(len(LAYOUTS))]


def _case_id(case):
    codec, (dtype, predictor), bands, layout = case
    return f"{codec}-{np.dtype(dtype).name}-p{predictor}-b{bands}-" + "x".join(str(v) for v in np.ravel(list(layout.values())))


@pytest.mark.parametrize("case", FILE_CASES, ids=_case_id)
def test_planar_files_decode_to_the_source_and_the_host_readers_pixels(tmp_path, case):
    codec, (dtype, predictor), bands, layout = case
    img = _raster(bands, 157, 683, dtype, seed=bands)
    path = str(tmp_path / "p.tif")
    _write(path, img, compression=codec, predictor=predictor, **layout)
    got, check = _decode(path)
    assert got.shape == (157, 683, bands) and got.dtype == img.dtype
    assert np.array_equal(_bytes(got.transpose(2, 0, 1)), _bytes(img))
    assert np.array_equal(_bytes(got.transpose(2, 0, 1)), _bytes(GeoTiff(path).read()))


@pytest.mark.parametrize("codec", ["lzw", "deflate", "zstd"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_a_wide_raster_in_short_strips(tmp_path, codec, dtype):
    """9 x 2100 in strips of 4 rows, predictor 2: rows of several steps, a last strip of one row."""
    img = _raster(4, 9, 2100, dtype, seed=3)
    path = str(tmp_path / "wide.tif")
    _write(path, img, compression=codec, predictor=2, rows_per_strip=4)
    got, _ = _decode(path)
    assert np.array_equal(_bytes(got.transpose(2, 0, 1)), _bytes(img))
    assert np.array_equal(_bytes(got.transpose(2, 0, 1)), _bytes(GeoTiff(path).read()))


# ---- 3. plane subsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("kw", [{"compression": "lzw", "tile": (64, 256), "predictor": 2}, {"compression": "deflate", "rows_per_strip": 7}])
def test_a_band_subset_reads_and_decodes_only_its_planes(tmp_path, dtype, kw):
    img = _raster(4, 157, 683, dtype, seed=8)
    path = str(tmp_path / "p.tif")
    _write(path, img, **kw)
    _, whole = _decode(path)
    for bands in ((0, 3), (2,), (0, 1, 2), (0,)):
        got, check = _decode(path, bands=bands)
        assert got.shape == (157, 683, 4)
        for c in range(4):
            assert np.array_equal(got[:, :, c], img[c] if c in bands else np.zeros_like(img[c])), (bands, c)
        assert check.compressed_bytes < whole.compressed_bytes
    assert 2 * check.compressed_bytes < whole.compressed_bytes      # bands=(0,): one plane of four similar ones
    # a pixel-interleaved file has no planes to pick
    chunky = str(tmp_path / "c.tif")
    write_geotiff(chunky, img, T, 25832, **kw)
    for planar in (False, True):
        with pytest.raises(ValueError, match="bands"):
            GeoTiff(chunky).decode_to_device("cuda:0", planar=planar, bands=(0, 3))
    # and a planar file without the keyword is refused as ever
    with pytest.raises(ValueError, match="not decodable on the device"):
        GeoTiff(path).decode_to_device("cuda:0")


# ---- 3b. the steps by hand, as the measuring tool composes them ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar_deflate_u8_bands03", "chunky_lzw_u16_p2_strips"])
def test_the_steps_called_by_hand_give_decode_to_devices_image(tmp_path, name):
    """device_block_plan → stage_offsets → alloc_block_buffers → launch_block_decoder → launch_layout (tools/raster_decode_bench.py times
    the launches through these calls): the same bytes as decode_to_device and the host reader, every block's status 0."""
    path = str(tmp_path / "s.tif")
    if name.startswith("planar"):
        img, bands = np.random.default_rng(0).integers(0, 256, (4, 80, 112), dtype=np.uint8), (0, 3)
        write_geotiff(path, img, T, 25832, compression="deflate", planar=True, tile=(32, 48))
    else:
        img, bands = np.random.default_rng(1).integers(0, 65536, (3, 61, 83), dtype=np.uint16), None
        write_geotiff(path, img, T, 25832, compression="lzw", predictor=2, rows_per_strip=7)
    g = GeoTiff(path)
    planes, mask, offs, cnts, expect, ranges = g.device_block_plan(bands)
    assert len(ranges) == (2 if bands else 1)
    rel, starts, span = D.stage_offsets(offs, ranges)
    raw = np.fromfile(path, dtype=np.uint8)
    comp = torch.from_numpy(np.concatenate([raw[lo:hi] for lo, hi in ranges] + [np.zeros(16, np.uint8)])).cuda()
    assert comp.numel() == span + 16
    meta = torch.from_numpy(np.stack([rel, cnts])).cuda()
    nb, cap = len(offs), g._bw * g._bh * (g.count if g.planar == 1 else 1) * g.dtype.itemsize
    bufs = D.alloc_block_buffers(g.compression, nb, cap, "cuda")
    assert bufs.blocks.shape == (nb, cap) and bufs.decoded.shape == (nb,) and bufs.status.shape == (2 * nb + 1,)
    image = torch.empty((g.height, g.width, g.count), dtype={1: torch.uint8, 2: torch.uint16}[g.dtype.itemsize], device="cuda")
    sp = _lib.stream_ptr()
    D.launch_block_decoder(g.compression, comp, meta, bufs, sp)
    D.launch_layout(bufs.blocks, cap, g._bw, g._bh, g._nx, g._ny, g.count, g._predictor, image, g.width, g.height, sp,
                    mask if g.planar == 2 else None)
    torch.cuda.synchronize()
    assert not bufs.status[:nb].cpu().numpy().any()
    assert np.array_equal(bufs.decoded.cpu().numpy() & 0xffffffff, expect)
    got = image.cpu().numpy()
    _, check = GeoTiff(path).decode_to_device("cuda:0", planar=g.planar == 2, bands=bands)
    assert np.array_equal(_bytes(got), _bytes(check().cpu().numpy()))
    host = GeoTiff(path).read()
    for c in range(g.count):
        want = host[c] if bands is None or c in bands else np.zeros_like(host[c])
        assert np.array_equal(_bytes(got[:, :, c]), _bytes(want)), c
    assert np.array_equal(host, img)


# ---- 4. more blocks than decoder waves -------------------------------------------------------------------------------------------------
def test_more_blocks_than_decoder_waves_go_by_ticket(tmp_path, monkeypatch):
    """4 planes x 900 one-row strips = 3 600 blocks: more than the chip holds decoder waves, so every wave fetches several blocks from
    the launch's counter; two decodes in a row take fresh counters."""
    monkeypatch.delenv("TD_DECODE_RING", raising=False)
    img = _raster(4, 900, 96, np.uint8, seed=4)
    for codec in ("lzw", "deflate"):
        path = str(tmp_path / f"ticket_{codec}.tif")
        _write(path, img, compression=codec, rows_per_strip=1, predictor=2)
        for _ in range(2):
            got, _ = _decode(path)
            assert np.array_equal(got.transpose(2, 0, 1), img), codec


# ---- 5. a damaged block, 6. the Predictor ---------------------------------------------------------------------------------------------
def test_a_corrupt_block_in_plane_2_is_reported_and_the_predictor_falls_back(tmp_path, capsys):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    img = _raster(3, 500, 500, np.uint8, seed=9)
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    _write(good, img, compression="lzw", tile=(128, 128))
    g = GeoTiff(good)
    g._setup_blocks()
    assert len(g._offs) == 3 * 16
    raw = bytearray(open(good, "rb").read())
    off = g._offs[2 * 16 + 5]                                       # block 5 of plane 2: block 37 of the file
    raw[off + 2: off + 6] = b"\xff\xff\xff\xff"                     # codes beyond the table
    open(bad, "wb").write(bytes(raw))
    image, check = GeoTiff(bad).decode_to_device("cuda:0", planar=True)
    with pytest.raises(ValueError, match="block 37"):
        check()
    image, check = GeoTiff(bad).decode_to_device("cuda:0", planar=True, bands=(2,))     # the file's number, whatever was left out
    with pytest.raises(ValueError, match="block 37"):
        check()
    image, check = GeoTiff(bad).decode_to_device("cuda:0", planar=True, bands=(0, 1))   # the damaged plane is not even read
    assert np.array_equal(check().cpu().numpy()[:, :, :2].transpose(2, 0, 1), img[:2])
    tile_single_file(bad, str(tmp_path / "tiles"), buffer=0, tile_width=25, tile_height=25)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    outs = {}
    for planar in (True, False):
        out = tmp_path / f"out_{planar}"
        with TD.Predictor(cfg, device_type="0", max_batch_size=4, output_dir=str(out), state_dict=sd, device_decode_planar=planar) as pred:
            pred(bad, str(tmp_path / "tiles" / "bad.json"))
            assert pred.decode_stats["images"] == 0
        text = capsys.readouterr().out
        assert ("using the host reader" in text) == planar, text
        files = sorted(os.listdir(out / "bad"))
        assert 0 < len(files) < 16
        outs[planar] = {f: open(out / "bad" / f, "rb").read() for f in files}
    assert outs[True] == outs[False]


@pytest.mark.parametrize("name", ["lzw_u8x4", "deflate_u16x3"])
def test_prediction_files_are_identical_with_device_decode_planar_on_or_off(tmp_path, name):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    rgb, _ = make_tile(300, 500)
    rgbi = np.ascontiguousarray(np.concatenate([rgb, rgb[..., 1:2]], axis=2).transpose(2, 0, 1))
    if name == "lzw_u8x4":
        img, kw = rgbi, {"compression": "lzw", "tile": (128, 128), "predictor": 2}
    else:
        img, kw = (rgbi[:3].astype(np.uint16) * 257), {"compression": "deflate", "rows_per_strip": 3, "predictor": 2}
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    outs = {}
    for planar in (True, False, "absent"):
        d = tmp_path / f"{planar}"
        (d / "rgb").mkdir(parents=True)
        tif = str(d / "rgb" / "9.tif")
        _write(tif, img, **kw)
        tile_single_file(tif, str(d / "tiles"), buffer=10, tile_width=40, tile_height=40)
        extra = {} if planar == "absent" else {"device_decode_planar": planar}
        with TD.Predictor(cfg, device_type="0", max_batch_size=3, output_dir=str(d / "out"), state_dict=sd, **extra) as pred:
            pred.prefetch(tif)
            pred(tif, str(d / "tiles" / "9.json"))
            if planar is True:
                assert pred.decode_stats["images"] >= 1, pred.decode_stats
            else:
                assert pred.decode_stats["images"] == 0 and pred.upload_stats["images"] == 0, pred.decode_stats
        files = sorted(os.listdir(d / "out" / "9"))
        outs[planar] = {f: open(d / "out" / "9" / f, "rb").read().replace(tif.encode(), b"IMG") for f in files}
        assert len(files) == 9
    assert outs[True] == outs[False] == outs["absent"]
    assert sum(len(json.loads(v)) for v in outs[True].values()) > 5


# ---- 7. the crown stage --------------------------------------------------------------------------------------------------------------
SIDE = 300
CT = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318060.0)
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318060.0)


def _scene(seed=9):
    """An RGBI image (0.2 m, 300 x 300), an nDSM on a 1 m grid (60 x 60) with blob crowns of known height, their rings and scores."""
    rng = np.random.default_rng(seed)
    rgbi = rng.integers(40, 120, (4, SIDE, SIDE), dtype=np.uint8)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    fine = rng.uniform(0, 1.0, (SIDE, SIDE)).astype(np.float32)
    rings = []
    for k in range(14):
        cx, cy, r = rng.uniform(30, 270), rng.uniform(30, 270), rng.uniform(8, 25)
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        inside = d2 < r ** 2
        rgbi[3][inside] = 220 if k % 4 else 60
        hgt = float(rng.uniform(1.0, 25.0))
        fine[inside] = np.maximum(fine[inside], hgt * (1 - d2[inside] / r ** 2 * 0.5))
        ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        ring = np.stack([CT[2] + CT[0] * (cx + r * np.cos(ang)), CT[5] + CT[4] * (cy + r * np.sin(ang))], axis=1)
        rings.append(np.concatenate([ring, ring[:1]]))
    ndsm = fine.reshape(60, 5, 60, 5).max(axis=(1, 3)).astype(np.float32)
    return rgbi, ndsm, rings, [0.95 - 0.03 * k for k in range(len(rings))]


def _config(device_decode, planar, n_scale):
    cfg = {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 3,
           "ndvi_mean_threshold": 0.2, "ndvi_var_threshold": 0.5, "use_overlap": False, "tile_width": 50, "tile_height": 50, "buffer": 10,
           "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": n_scale, "height_scaling_factor": 1.0,
           "device_decode": device_decode}
    if planar is not None:
        cfg["device_decode_planar"] = planar
    return cfg


def _same_features(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


def _no_host_reader(self):
    raise AssertionError(f"{self.path} went through the host reader")


@pytest.mark.parametrize("n_scale", [1.0, 0.2])
def test_process_layer_is_the_same_with_planar_rasters_on_the_device(tmp_path, monkeypatch, n_scale):
    rgbi, ndsm, rings, scores = _scene()
    rpath, hpath = str(tmp_path / "rgbi.tif"), str(tmp_path / "ndsm.tif")
    _write(rpath, rgbi, CT, compression="deflate", tile=(128, 128), predictor=2)
    _write(hpath, ndsm[None], NT, compression="deflate", predictor=3, tile=(32, 32))
    # one band, yet band-separate by its tag: the height raster takes the planar path
    assert GeoTiff(hpath).planar == 2 and GeoTiff(rpath).planar == 2
    host = P.process_layer(rings, scores, _config(False, None, n_scale), hpath, rpath)
    assert len(host) >= 3 and any(f["properties"]["TreeHeight"] > 3 for f in host)
    P.ndvi_decode_stats.update(planes=0, compressed_bytes=0)
    with monkeypatch.context() as m:
        m.setattr(GeoTiff, "read", _no_host_reader)         # neither raster may take the host route
        dev = P.process_layer(rings, scores, _config(True, True, n_scale), hpath, rpath)
    _same_features(host, dev)
    # NDVI asked for the red and the infrared plane only: what went to the device is those two planes' blocks
    g = GeoTiff(rpath)
    want = sum(hi - lo for lo, hi in g.device_block_plan(bands=(0, 3))[5])
    assert P.ndvi_decode_stats == {"planes": 2, "compressed_bytes": want}
    assert want < 0.75 * sum(hi - lo for lo, hi in g.device_block_plan()[5])
    # the key off or absent, or device_decode left at "auto": the host reader, as before
    for cfg in (_config(True, False, n_scale), _config(True, None, n_scale), _config("auto", True, n_scale)):
        with monkeypatch.context() as m:
            m.setattr(GeoTiff, "decode_to_device", lambda *a, **k: pytest.fail("the device path ran"))
            _same_features(host, P.process_layer(rings, scores, cfg, hpath, rpath))
