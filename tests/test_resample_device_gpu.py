"""td_resample_gdal_dev (resample.hip) — GDAL's triangle-filter resampler and the NDVI rule on a raster in HBM — against the host
functions that define the values: postprocessing.resample_bilinear_gdal for uint8 (mode u8), the float64 evaluation of the same
float32 taps for float32 (mode f32), ndvi_from_rgbi bit for bit over all 65 536 (red, near-infrared) pairs (mode ndvi); guarded
memory around tmp and dst; the refusals of the entry point and of the Python wrapper."""
import ctypes as C

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff

from resample_cases import CASES, eval64_f32, eval64_u8, f32_bound, f32_raster, host_u8, u8_raster

pytestmark = pytest.mark.gpu


def _interleaved(chw):
    """[bands, rows, cols] numpy → CUDA [rows, cols, bands], the layout GeoTiff.decode_to_device returns."""
    return torch.from_numpy(np.ascontiguousarray(chw.transpose(1, 2, 0))).cuda()


@pytest.mark.parametrize("name", sorted(CASES))
def test_uint8_rasters_equal_the_host_function(name):
    """Equal at every pixel whose float64 evaluation lies at least 1e-3 from a rounding boundary k + 0.5; inside that band at most
    one level apart; the band holds at most 1 % of the pixels (a condition on the case, asserted)."""
    h, w, out_h, out_w = CASES[name]
    src = _interleaved(u8_raster(name))
    ref, exact = host_u8(name), eval64_u8(name)
    frac = exact + 0.5 - np.floor(exact + 0.5)                 # distance above the boundary below, in [0, 1)
    near = np.minimum(frac, 1.0 - frac) < 1e-3
    print(f"{name}: {near.mean() * 100:.3f} % of the pixels within 1e-3 of a rounding boundary")
    assert near.mean() <= 0.01
    for bands in ([0, 1, 2, 3], [0, 3]):
        got = P.resample_on_device(src, out_h, out_w, bands, "u8")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(bands), out_h, out_w) and got.is_cuda
        got = got.cpu().numpy().astype(np.int32)
        diff = np.abs(got - ref[bands].astype(np.int32))
        print(f"{name} bands {bands}: {int((diff != 0).sum())} pixels differ from the host function, largest difference {int(diff.max())}")
        assert (diff[~near[bands]] == 0).all()
        assert (diff[near[bands]] <= 1).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_rasters_stay_within_the_bound_of_two_sequential_sums(name):
    h, w, out_h, out_w = CASES[name]
    img = f32_raster(name)
    got = P.resample_on_device(torch.from_numpy(img[0].copy()).cuda(), out_h, out_w, [0], "f32")
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, out_h, out_w)
    err = np.abs(got.cpu().numpy().astype(np.float64) - eval64_f32(name)).max()
    bound = f32_bound(h, w, out_h, out_w, np.abs(img).max())
    print(f"{name}: largest error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _all_pairs():
    x = np.zeros((4, 256, 256), np.uint8)
    x[0] = np.arange(256, dtype=np.uint8)[:, None]          # red: the row
    x[3] = np.arange(256, dtype=np.uint8)[None, :]          # near-infrared: the column
    x[1], x[2] = 77, 201
    return x


def test_ndvi_of_all_band_pairs_bit_for_bit(tmp_path):
    x = _all_pairs()
    ref = P.ndvi_from_rgbi(x).astype(np.float32)
    assert ref[0, 0] == 0.0                                  # 0 / 1e-10
    got = P.resample_on_device(_interleaved(x), 256, 256, [0, 3], "ndvi")      # identity taps: weights (1, 0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (256, 256)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    # the same through the crown stage's own entry, from an LZW file
    path = str(tmp_path / "pairs.tif")
    write_geotiff(path, x, (0.2, 0.0, 412000.0, 0.0, -0.2, 5318060.0), 25832, compression="lzw", predictor=2, rows_per_strip=16)
    rg = GeoTiff(path)
    staged = P._ndvi_on_device(rg, 1.0, {"device_decode": True}, 0)
    assert staged is not None and staged.is_cuda and np.array_equal(staged.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    for off in (False, "auto", None):
        assert P._ndvi_on_device(rg, 1.0, {"device_decode": off}, 0) is None
    assert P._ndvi_on_device(rg, 1.0, {}, 0) is None
    rg.close()


GUARD = 1 << 16
SENTINEL = 0xDEADBEEF


def _upload(table):
    return [torch.from_numpy(a).cuda() for a in table]


def _raw(src, sample, h, w, c, bands, xt, yt, d_x, d_y, tmp, dst, mode):
    lib = _lib.load()
    band_list = (C.c_int32 * len(bands))(*bands)
    return lib.td_resample_gdal_dev(src.data_ptr(), sample, h, w, c, band_list, len(bands), *[a.data_ptr() for a in d_x], len(xt[0]), xt[3].size,
                                    *[a.data_ptr() for a in d_y], len(yt[0]), yt[3].size, tmp.data_ptr(), dst.data_ptr(), mode, _lib.stream_ptr())


@pytest.mark.parametrize("mode", ["u8", "f32"])
@pytest.mark.parametrize("name", ["203x317@0.2", "97x131@1.7"])
def test_nothing_is_written_outside_tmp_and_dst(name, mode):
    """tmp and dst lie in the middle of sentinel-filled buffers, 64 Ki elements on either side: the guards still hold the sentinel
    afterwards and the middle holds what the wrapper (its own allocations) returns."""
    h, w, out_h, out_w = CASES[name]
    if mode == "u8":
        src, bands, sample, c = _interleaved(u8_raster(name)), [0, 1, 2, 3], _lib.SAMPLE_U8, 4
    else:
        src, bands, sample, c = torch.from_numpy(f32_raster(name)[0].copy()).cuda(), [0], _lib.SAMPLE_F32, 1
    nb = len(bands)
    xt, yt = P.tap_tables(w, out_w), P.tap_tables(h, out_h)
    d_x, d_y = _upload(xt), _upload(yt)
    n_tmp, n_dst = nb * h * out_w, nb * out_h * out_w
    tmp_buf = torch.full((GUARD + n_tmp + GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    if mode == "u8":
        dst_buf = torch.full((GUARD + n_dst + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    else:
        dst_buf = torch.full((GUARD + n_dst + GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    st = _raw(src, sample, h, w, c, bands, xt, yt, d_x, d_y, tmp_buf[GUARD:], dst_buf[GUARD:], _lib.RESAMPLE_MODES[mode])
    _lib.check(st, "td_resample_gdal_dev")
    torch.cuda.synchronize()
    t = tmp_buf.cpu().numpy().view(np.uint32)
    assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + n_tmp:] == SENTINEL).all()
    d = dst_buf.cpu().numpy()
    guard_value = 0xA5 if mode == "u8" else SENTINEL
    d = d if mode == "u8" else d.view(np.uint32)
    assert (d[:GUARD] == guard_value).all() and (d[GUARD + n_dst:] == guard_value).all()
    want = P.resample_on_device(src, out_h, out_w, bands, mode).cpu().numpy()
    assert np.array_equal(d[GUARD:GUARD + n_dst], want.reshape(-1) if mode == "u8" else want.reshape(-1).view(np.uint32))


def test_the_entry_point_refuses_before_any_launch():
    """Every refusal returns TD_ERR_INVALID with a message and leaves tmp and dst untouched (nothing ran)."""
    lib = _lib.load()
    h, w, out_h, out_w = 20, 30, 4, 6
    xt, yt = P.tap_tables(w, out_w), P.tap_tables(h, out_h)
    d_x, d_y = _upload(xt), _upload(yt)
    u8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    f32 = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    tmp = torch.full((4 * h * out_w,), 7.0, dtype=torch.float32, device="cuda")
    dst = torch.full((4 * out_h * out_w,), 7.0, dtype=torch.float32, device="cuda")
    U8, F32 = _lib.SAMPLE_U8, _lib.SAMPLE_F32
    M = _lib.RESAMPLE_MODES
    assert _raw(u8, U8, h, w, 4, [0, 3], xt, yt, d_x, d_y, tmp, dst, M["ndvi"]) == 0
    torch.cuda.synchronize()
    tmp.fill_(7.0)
    dst.fill_(7.0)
    refused = [
        ("band index 4", (u8, U8, h, w, 4, [0, 4], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
        ("band index 3", (u8, U8, h, w, 3, [0, 3], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
        ("band index 1", (f32, F32, h, w, 1, [1], xt, yt, d_x, d_y, tmp, dst, M["f32"])),
        ("exactly two bands", (u8, U8, h, w, 4, [0, 1, 3], xt, yt, d_x, d_y, tmp, dst, M["ndvi"])),
        ("exactly two bands", (u8, U8, h, w, 4, [3], xt, yt, d_x, d_y, tmp, dst, M["ndvi"])),
        ("source is float32", (f32, F32, h, w, 1, [0], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
        ("source is float32", (f32, F32, h, w, 1, [0, 0], xt, yt, d_x, d_y, tmp, dst, M["ndvi"])),
        ("samples per pixel", (u8, U8, h, w, 5, [0], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
        ("samples per pixel", (f32, F32, h, w, 2, [0], xt, yt, d_x, d_y, tmp, dst, M["f32"])),
        ("output mode 3", (u8, U8, h, w, 4, [0], xt, yt, d_x, d_y, tmp, dst, 3)),
        ("sample type 2", (u8, 2, h, w, 4, [0], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
        ("0 x 30 source", (u8, U8, 0, w, 4, [0], xt, yt, d_x, d_y, tmp, dst, M["u8"])),
    ]
    for message, args in refused:
        assert _raw(*args) == _lib.ERR_INVALID, message
        assert message in lib.td_last_error().decode(), (message, lib.td_last_error())
    band_list = (C.c_int32 * 2)(0, 3)
    ok = [u8.data_ptr(), U8, h, w, 4, band_list, 2, *[a.data_ptr() for a in d_x], out_w, xt[3].size, *[a.data_ptr() for a in d_y], out_h, yt[3].size,
          tmp.data_ptr(), dst.data_ptr(), M["ndvi"], _lib.stream_ptr()]
    for k, v in ((0, None), (5, None), (6, 0), (6, 5), (7, None), (10, None), (11, 0), (12, 0), (13, None), (16, None), (17, 0), (18, 0), (19, None), (20, None)):
        bad = list(ok)
        bad[k] = v
        assert lib.td_resample_gdal_dev(*bad) == _lib.ERR_INVALID, (k, v)
    torch.cuda.synchronize()
    assert (tmp == 7.0).all() and (dst == 7.0).all()


def test_the_wrapper_refuses_a_table_that_reaches_outside_the_source():
    src = _interleaved(u8_raster("64x64@0.37"))
    good = P.tap_tables(64, 23)
    for k, (j, v) in (("start", (22, 61)), ("start", (0, -1)), ("count", (22, 8)), ("count", (3, 0)), ("offset", (22, 10 ** 6))):
        bad = dict(zip(("start", "count", "offset", "weights"), (a.copy() for a in good)))
        bad[k][j] = v
        bad = tuple(bad.values())
        for tables in ((bad, good), (good, bad)):
            with pytest.raises(ValueError, match="tap table reaches outside"):
                P.resample_on_device(src, 23, 23, [0, 3], "ndvi", tables=tables)
    for bands, mode in (([0, 4], "u8"), ([0, 1, 3], "ndvi"), ([], "u8")):
        with pytest.raises(_lib.TdError, match="td_resample_gdal_dev"):
            P.resample_on_device(src, 23, 23, bands, mode)
    with pytest.raises(_lib.TdError, match="source is float32"):
        P.resample_on_device(torch.zeros((8, 8), dtype=torch.float32, device="cuda"), 4, 4, [0], "u8")
    torch.cuda.synchronize()
