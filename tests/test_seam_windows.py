"""The host side of the device seam strips (treedetection_amd/merging.py ``device_seams``): the windowed block plan of
``GeoTiff.device_block_plan`` against a brute-force overlap test, ``seam_windows`` against the oracle's mosaic + centre crop, and the
config key. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.merging_ref import crop_center_ref, merge_images_ref  # noqa: E402
from treedetection_amd.geotiff import GeoTiff, write_geotiff  # noqa: E402
from treedetection_amd.merging import device_seams_setting, merge_and_crop_images, seam_windows  # noqa: E402

from seam_cases import GEOMETRY, first_rule, rand_raster, windows  # noqa: E402

T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318000.0)
H, W = 37, 50                                                   # a 50 x 37 px raster: 16-px tiles leave a partly filled last column and row,
LAYOUTS = [{"tile": (16, 16)}, {"tile": (32, 16)}, {"rows_per_strip": 5}]     # 5-row strips a short last strip of 2 rows


def _file(tmp_path, layout, planar, dtype=np.uint8, bands=3):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 255, (bands, H, W)).astype(dtype)
    path = str(tmp_path / "r.tif")
    write_geotiff(path, img, T, 25832, compression="deflate", planar=planar, **layout)
    g = GeoTiff(path)
    g._setup_blocks()
    return g


def _merged(spans):
    """Byte spans, ascending, joined where they overlap or lie within 4 KB of each other."""
    spans = sorted(spans)
    out = [spans[0]]
    for lo, hi in spans[1:]:
        if lo <= out[-1][1] + 4096:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _bytes(ranges):
    return sum(hi - lo for lo, hi in ranges)


def _brute_force(g, planes, window):
    """Every block of the file whose pixels intersect the window, plane after plane, row-major → (file indices, expect, sub-grid)."""
    r0, c0, h, w = window
    hit = [(by, bx) for by in range(g._ny) for bx in range(g._nx)
           if by * g._bh < r0 + h and min((by + 1) * g._bh, g.height) > r0 and bx * g._bw < c0 + w and min((bx + 1) * g._bw, g.width) > c0]
    bys, bxs = sorted({b[0] for b in hit}), sorted({b[1] for b in hit})
    assert hit == [(by, bx) for by in bys for bx in bxs]         # a rectangle of the grid
    cb = g.count if g.planar == 1 else 1
    rows = lambda by: min(g._bh, g.height - by * g._bh) if g._strips else g._bh
    idx = [p * g._nx * g._ny + by * g._nx + bx for p in planes for by, bx in hit]
    expect = [rows(by) * g._bw * cb * g.dtype.itemsize for _ in planes for by, _ in hit]
    return idx, expect, (bys[0], bxs[0], len(bys), len(bxs))


@pytest.mark.parametrize("planar", [False, True], ids=["chunky", "planar"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["t16x16", "t32x16", "s5"])
def test_the_windowed_plan_lists_the_blocks_the_window_overlaps(tmp_path, layout, planar):
    g = _file(tmp_path, layout, planar)
    offs_all, cnts_all = np.asarray(g._offs, dtype=np.int64), np.asarray(g._counts, dtype=np.int64)
    short_last = g._strips and g.height % g._bh
    for bands in ([None] + ([(2,), (2, 0)] if planar else [])):
        planes_want = [0] if not planar else sorted(range(g.count) if bands is None else bands)
        for name, window in windows(H, W, g._bh, g._bw).items():
            planes, mask, offs, cnts, expect, ranges, sub = g.device_block_plan(bands, window)
            idx, expect_want, sub_want = _brute_force(g, planes_want, window)
            assert planes == planes_want and mask == (sum(1 << p for p in planes) if planar else 1), name
            assert sub == sub_want, (name, sub, sub_want)
            assert offs.dtype == np.int64 and np.array_equal(offs, offs_all[idx]) and np.array_equal(cnts, cnts_all[idx]), name
            assert np.array_equal(expect, expect_want), name
            if short_last and name in ("end", "whole"):
                assert expect[-1] == (g.height % g._bh) * g._bw * (1 if planar else g.count), name       # the short last strip
            # the ranges: ascending, apart, and every listed block inside one of them; nothing but listed blocks and the gaps between
            # neighbours is read — never more than one range per plane would
            assert all(lo < hi for lo, hi in ranges) and all(a[1] < b[0] for a, b in zip(ranges, ranges[1:])), ranges
            assert all(any(lo <= o and o + n <= hi for lo, hi in ranges) for o, n in zip(offs, cnts)), name
            per = len(offs) // len(planes)
            one_per_plane = _merged((int(offs[i:i + per].min()), int((offs + cnts)[i:i + per].max())) for i in range(0, len(offs), per))
            assert int(cnts.sum()) <= _bytes(ranges) <= _bytes(one_per_plane), (name, ranges)
        # without a window: what it always returned — six entries, every block of the selected planes, one range per plane before merging
        plan = g.device_block_plan(bands)
        assert len(plan) == 6
        planes, mask, offs, cnts, expect, ranges = plan
        idx, expect_want, sub_want = _brute_force(g, planes_want, (0, 0, H, W))
        assert sub_want == (0, 0, g._ny, g._nx) and planes == planes_want
        assert np.array_equal(offs, offs_all[idx]) and np.array_equal(cnts, cnts_all[idx]) and np.array_equal(expect, expect_want)
        per = g._nx * g._ny
        assert ranges == _merged((int(offs[i:i + per].min()), int((offs + cnts)[i:i + per].max())) for i in range(0, len(offs), per))
        whole = g.device_block_plan(bands, (0, 0, H, W))
        assert all(np.array_equal(a, b) for a, b in zip(whole[2:5], plan[2:5])) and whole[6] == (0, 0, g._ny, g._nx)


def test_a_narrow_window_of_a_tiled_file_reads_a_range_per_block_row(tmp_path):
    """Tiles of 12 KB: the three tiles between two block rows of the window's column are further than the 4 KB that ranges bridge."""
    path = str(tmp_path / "big.tif")
    write_geotiff(path, np.random.default_rng(1).integers(0, 255, (3, 200, 250)).astype(np.uint8), T, 25832, compression="deflate", tile=(64, 64))
    g = GeoTiff(path)
    _, _, offs, cnts, _, ranges, sub = g.device_block_plan(None, (0, 70, 200, 3))        # block column 1, all four block rows
    assert sub == (0, 1, 4, 1) and len(ranges) == 4
    assert ranges == [(int(o), int(o + n)) for o, n in zip(offs, cnts)]
    assert _bytes(ranges) * 3 < int((offs + cnts).max() - offs.min())                    # what one range for the plane would read


@pytest.mark.parametrize("window", [(0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, H + 1, 1), (H - 1, W - 1, 2, 1), (H - 1, W - 1, 1, 2),
                                    (H, 0, 1, 1), (0, 0, 1), (0.5, 0, 1, 1), "abcd"], ids=str)
def test_bad_windows_are_refused_by_name(tmp_path, window):
    g = _file(tmp_path, {"tile": (16, 16)}, False)
    with pytest.raises(ValueError, match="window"):
        g.device_block_plan(None, window)


# ---- seam_windows against the oracle ---------------------------------------------------------------------------------------------------
def _pair(tmp_path, k, case, rng):
    dtype, bands, s1, s2, (dx, dy), nd, zf = case
    a1, a2 = rand_raster(rng, bands, s1[0], s1[1], dtype, zf), rand_raster(rng, bands, s2[0], s2[1], dtype, zf)
    if nd is not None and abs(nd) < 1e10:
        a1[:, rng.random(s1) < 0.2] = nd
    gsd = 0.2
    t1 = (gsd, 0.0, 412000.0, 0.0, -gsd, 5318000.0)
    t2 = (gsd, 0.0, 412000.0 + dx * gsd, 0.0, -gsd, 5318000.0 - dy * gsd)
    p1, p2 = str(tmp_path / f"a{k}.tif"), str(tmp_path / f"b{k}.tif")
    write_geotiff(p1, a1, t1, 25832, nodata=nd)
    write_geotiff(p2, a2, t2, 25832)
    return (a1, t1, GeoTiff(p1)), (a2, t2, GeoTiff(p2)), nd


@pytest.mark.parametrize("horizontal", [True, False], ids=["right", "bottom"])
@pytest.mark.parametrize("k", range(len(GEOMETRY)))
def test_seam_windows_cut_what_the_oracle_crops_out_of_its_mosaic(tmp_path, k, horizontal):
    (a1, t1, g1), (a2, t2, g2), nd = _pair(tmp_path, k, GEOMETRY[k], np.random.default_rng(7 + k))
    ref, rt = merge_images_ref(a1, t1, a2, t2, nd)
    cfg = {"tile_width": 4, "tile_height": 3, "buffer": 1, "overlapping_tiles_width": 2, "overlapping_tiles_height": 3}
    cw, ch = ((4 + 2) * 2, ref.shape[1]) if horizontal else (ref.shape[2], (3 + 2) * 3)
    want = crop_center_ref(ref, rt, cw, ch)
    assert want is not None
    reads = []
    for g in (g1, g2):
        g.read = g._window_hwc = lambda *a, **kw: reads.append(1)           # the geometry comes from the transforms and sizes alone
    geo = seam_windows(g1, g2, horizontal, cfg)
    assert not reads
    assert geo.mosaic == ref.shape[1:] and np.allclose(geo.mosaic_transform, rt, rtol=0, atol=1e-9)
    top, left, rows, cols = geo.strip
    assert (rows, cols) == want[0].shape[1:] and np.allclose(geo.transform, want[1], rtol=0, atol=1e-9)
    assert (left, top) == (max(ref.shape[2] // 2 - cw // 2, 0), max(ref.shape[1] // 2 - ch // 2, 0))
    parts = []
    for (arr, _, g), part, own in zip(((a1, t1, g1), (a2, t2, g2)), geo.sources, (nd, None)):
        if part is None:
            continue
        (r0, c0, h, w), at = part
        assert 0 <= r0 and 0 <= c0 and h >= 1 and w >= 1 and r0 + h <= g.height and c0 + w <= g.width
        parts.append((arr[:, r0:r0 + h, c0:c0 + w].transpose(1, 2, 0), at, own))
    assert parts
    strip = first_rule(np.empty((rows, cols, a1.shape[0]), dtype=a1.dtype), geo.fill, parts)
    assert strip.dtype == want[0].dtype and np.ascontiguousarray(strip.transpose(2, 0, 1)).tobytes() == np.ascontiguousarray(want[0]).tobytes()


def test_a_strip_that_does_not_fit_raises_before_anything_is_read(tmp_path):
    (a1, t1, g1), (a2, t2, g2), nd = _pair(tmp_path, 0, GEOMETRY[0], np.random.default_rng(1))
    ref, rt = merge_images_ref(a1, t1, a2, t2, nd)
    cfg = {"tile_width": 4, "tile_height": 3, "buffer": 1, "overlapping_tiles_width": 40, "overlapping_tiles_height": 40}
    for horizontal, (cw, ch) in ((True, (240, ref.shape[1])), (False, (ref.shape[2], 200))):
        assert crop_center_ref(ref, rt, cw, ch) is None
        with pytest.raises(ValueError, match=f"crop window {cw}x{ch} .* exceeds the {ref.shape[2]}x{ref.shape[1]} mosaic"):
            seam_windows(g1, g2, horizontal, cfg)


def test_a_fill_value_beyond_the_dtype_warns_as_merge_images_does(tmp_path):
    rng = np.random.default_rng(5)
    p1, p2 = str(tmp_path / "a.tif"), str(tmp_path / "b.tif")
    write_geotiff(p1, rand_raster(rng, 3, 16, 16, np.uint8), T, 25832, nodata=-9999.0)
    write_geotiff(p2, rand_raster(rng, 3, 16, 16, np.uint8), (0.2, 0.0, 412000.0 + 16 * 0.2, 0.0, -0.2, 5318000.0), 25832)
    cfg = {"tile_width": 2, "tile_height": 2, "buffer": 1, "overlapping_tiles_width": 2, "overlapping_tiles_height": 2}
    with pytest.warns(UserWarning, match="beyond the valid range"):
        geo = seam_windows(GeoTiff(p1), GeoTiff(p2), True, cfg)
    assert geo.fill == 0.0 and geo.strip == (0, 12, 16, 8) and geo.sources == [((0, 12, 16, 4), (0, 0)), ((0, 0, 16, 4), (0, 4))]


# ---- the config key ---------------------------------------------------------------------------------------------------------------------
class Log:
    def __init__(self):
        self.msgs = []

    def __getattr__(self, name):
        return lambda m: self.msgs.append((name, m))


def test_device_seams_is_true_or_false_and_off_by_default(tmp_path):
    assert device_seams_setting() is False and device_seams_setting(None) is False
    assert device_seams_setting(False) is False and device_seams_setting("false") is False
    assert device_seams_setting(True) is True and device_seams_setting("true") is True
    for bad in ("auto", "yes", 1, 0, "all", []):
        with pytest.raises(ValueError, match="device_seams must be true or false"):
            device_seams_setting(bad)
    import yaml
    from treedetection_amd.config import get_config
    for sub in ("rgb", "ndsm"):
        (tmp_path / sub).mkdir()
    (tmp_path / "m.npz").write_bytes(b"x")
    base = {"image_directory": str(tmp_path / "rgb"), "height_data_path": str(tmp_path / "ndsm"), "combined_model": str(tmp_path / "m.npz"),
            "output_directory": str(tmp_path / "out")}
    for extra, want in (({}, False), ({"device_seams": True}, True)):
        (tmp_path / "config.yml").write_text(yaml.safe_dump({**base, **extra}))
        assert get_config(str(tmp_path / "config.yml"))[0]["device_seams"] is want
    example = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "example", "config.yml")))
    assert example.get("device_seams", False) is False
    # merge_and_crop_images: a bad value is refused before anything is written; absent = false = the same files
    rng = np.random.default_rng(2)
    outs = {}
    for sub, extra in (("absent", {}), ("false", {"device_seams": False}), ("bad", {"device_seams": "maybe"})):
        d = tmp_path / sub
        os.makedirs(d)
        names = []
        for ix in range(2):
            names.append(str(d / f"{100 + ix}_x.tif"))
            write_geotiff(names[-1], rand_raster(np.random.default_rng(ix), 4, 24, 32, np.uint8, 0.1),
                          (0.25, 0.0, 500000.0 + ix * 32 * 0.25, 0.0, -0.25, 5400000.0), 25832, compression="deflate", tile=(16, 16))
        cfg = {"logger": Log(), "merged_path": "merged", "tile_width": 4, "tile_height": 4, "buffer": 1, "overlapping_tiles_width": 2,
               "overlapping_tiles_height": 2, **extra}
        if sub == "bad":
            with pytest.raises(ValueError, match="device_seams"):
                merge_and_crop_images(cfg, names, [])
            assert len(names) == 2 and not os.path.exists(d / "merged")
            continue
        merge_and_crop_images(cfg, names, [])
        assert len(names) == 3 and not cfg["logger"].msgs
        outs[sub] = open(names[2], "rb").read()
    assert outs["absent"] == outs["false"]
