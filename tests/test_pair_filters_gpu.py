"""The crown stage's box-pair filters on the GPU (crownpairs.hip: td_crown_pairs_count / td_crown_pairs_fill, then the host greedy
pass) against oracle.postprocess_ref, bit for bit: kept lists, containment triples and the connected-pair rows on the case families
of pair_cases.py at sizes on both sides of the kernels' 256-row blocks and 1 024-column chunks; numpy's half arithmetic of the
area test on float16 bit patterns; and process_layer with ``device_filters: true`` against the host path."""
import functools

import numpy as np
import pytest

from oracle import postprocess_ref as O
from treedetection_amd import box_pairs as BP
from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import write_geotiff

import pair_cases

pytestmark = pytest.mark.gpu

CHUNK = 1024                                                # PAIR_CHUNK of crownpairs.hip; its workgroups own 256 rows
SIZES = [1, 2, 255, 256, 257, CHUNK + 1]


@functools.lru_cache(maxsize=None)
def _reference(family, n):
    """The case and what the oracle makes of it, computed once: (case, kept, containment triple, mask without its diagonal)."""
    case = pair_cases.make(family, n, seed=7)
    kept = O.filter_by_iou_and_area(case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold)
    triple = O.containment(case.bounds, case.containment_threshold)
    mask = pair_cases.oracle_mask(case)
    np.fill_diagonal(mask, False)
    return case, kept, triple, mask


def _rows(pairs, n):
    row_start, cols = pairs
    assert row_start.shape == (n + 1,) and row_start[0] == 0 and cols.shape == (row_start[-1],)
    return [np.sort(cols[row_start[i]:row_start[i + 1]]) for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", pair_cases.FAMILIES)
def test_kept_list_and_containment_equal_the_oracle(family, n, capsys):
    case, kept, triple, _ = _reference(family, n)
    got = P.filter_polygons_by_iou_and_area_device(case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold)
    assert got == kept
    assert P.containment_device(case.bounds, case.containment_threshold) == triple
    assert "using the host function" not in capsys.readouterr().out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", pair_cases.FAMILIES)
def test_connected_pair_rows_equal_the_oracle_mask(family, n):
    case, _, _, mask = _reference(family, n)
    bb = np.array([[np.float32(v) for v in b] for b in case.bounds], dtype=np.float32).reshape(-1, 4)
    pairs = P.connected_pairs_device(bb, np.array(case.areas, dtype=np.float16), np.float32(case.iou_threshold), np.float16(case.area_threshold))
    rows = _rows(pairs, n)
    for i in range(n):
        assert np.array_equal(rows[i], np.flatnonzero(mask[i])), (family, n, i)


def _half_area_values():
    """2 048 float16 areas by bit pattern: every subnormal step near 0, both zeros, runs of neighbours one ulp apart across the
    exponent range, repeated values, the largest finite half (65 504), inf and a NaN."""
    bits = [0x0000, 0x8000, 0x7bff, 0x7bff, 0x7bfe, 0x7c00, 0x7c00, 0x7e00]
    bits += list(range(0x0001, 0x0041))                     # subnormals 2^-24 .. 64 * 2^-24
    bits += list(range(0x03f0, 0x0410))                     # across the subnormal / normal border
    for e in range(1, 31, 2):                               # 16 consecutive patterns at 15 exponents, twice (equal values)
        bits += list(range((e << 10) + 0x3f8, (e << 10) + 0x408)) * 2
    rng = np.random.default_rng(11)
    bits += [int(b) for b in rng.integers(0x0001, 0x7c00, 2048 - len(bits))]
    assert len(bits) == 2048
    return rng.permutation(np.array(bits, dtype=np.uint16)).view(np.float16)


@pytest.mark.parametrize("threshold", [1, 3, 0.0999])
def test_half_arithmetic_of_the_area_test_is_numpys(threshold):
    """Identical boxes (IoU 1), so the mask is the area test alone: |a_i - a_j| / max(a_i, a_j) < threshold evaluated as numpy
    evaluates float16 — float32 operations, rounded to half after each."""
    ar = _half_area_values()
    n = ar.size
    bb = np.tile(np.array([412000.0, 5318000.0, 412004.0, 5318004.0], np.float32), (n, 1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        want = np.abs(ar[:, None] - ar) / np.maximum(ar[:, None], ar) < threshold
    np.fill_diagonal(want, False)
    assert want.any() and not want.all()
    rows = _rows(P.connected_pairs_device(bb, ar, np.float32(0.5), np.float16(threshold)), n)
    got = np.zeros((n, n), bool)
    for i, r in enumerate(rows):
        got[i, r] = True
    bad = np.argwhere(got != want)
    assert not len(bad), [(ar[i], ar[j], got[i, j]) for i, j in bad[:5]]


def test_the_limit_on_connected_pairs_is_where_it_says(monkeypatch, capsys):
    """MAX_DEVICE_PAIRS lowered to this case's own number of connected pairs: that many are stored, one fewer allowed declines
    after the count pass (nothing is filled) and the wrapper says so in one line."""
    case, kept, _, mask = _reference("b", 257)
    total = int(mask.sum())
    assert total > 2
    args = (case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold)
    monkeypatch.setattr(BP, "MAX_DEVICE_PAIRS", total)
    assert P.filter_polygons_by_iou_and_area_device(*args) == kept
    assert capsys.readouterr().out == ""
    monkeypatch.setattr(BP, "MAX_DEVICE_PAIRS", total - 1)
    bb = np.array(case.bounds, dtype=np.float32).reshape(-1, 4)
    assert P.connected_pairs_device(bb, np.array(case.areas, dtype=np.float16), np.float32(case.iou_threshold), np.float16(case.area_threshold)) is None
    assert P.filter_polygons_by_iou_and_area_device(*args) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and f"more than {total - 1} connected pairs" in out and "using the host function" in out


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import torch
    from treedetection_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    b = torch.zeros((4, 4), dtype=torch.float32, device=dev)
    a = torch.zeros(4, dtype=torch.float16, device=dev)
    c = torch.zeros(5, dtype=torch.int32, device=dev)
    rs = torch.zeros(5, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr()
    good_count = [b.data_ptr(), a.data_ptr(), 4, 0.5, 0x3c00, c.data_ptr(), 0.9, c.data_ptr(), c.data_ptr(), s]
    good_fill = [b.data_ptr(), a.data_ptr(), 4, 0.5, 0x3c00, rs.data_ptr(), c.data_ptr(), c.data_ptr(), s]
    for k, v in ((0, None), (1, None), (2, 0), (2, -3), (2, 65535 * CHUNK + 1), (7, None), (8, None), (0, b.data_ptr() + 4)):
        bad = list(good_count)
        bad[k] = v
        assert lib.td_crown_pairs_count(*bad) == _lib.ERR_INVALID, (k, v)
        assert b"td_crown_pairs_count" in lib.td_last_error()
    bad = list(good_count)
    bad[5] = bad[7] = bad[8] = None
    assert lib.td_crown_pairs_count(*bad) == _lib.ERR_INVALID
    for k, v in ((0, None), (1, None), (2, 0), (2, 65535 * CHUNK + 1), (5, None), (6, None), (7, None), (0, b.data_ptr() + 8)):
        bad = list(good_fill)
        bad[k] = v
        assert lib.td_crown_pairs_fill(*bad) == _lib.ERR_INVALID, (k, v)
        assert b"td_crown_pairs_fill" in lib.td_last_error()
    torch.cuda.synchronize()


# ---- process_layer on both paths (the scene of test_postprocessing_device_gpu.py, with duplicated and nested crowns) ----------
SIDE = 600                                                  # RGBI pixels of 0.2 m; the nDSM has SIDE / 5 pixels of 1 m
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318120.0)


def _ring(cx, cy, r):
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    ring = np.stack([T[2] + T[0] * (cx + r * np.cos(ang)), T[5] + T[4] * (cy + r * np.sin(ang))], axis=1)
    return np.concatenate([ring, ring[:1]])


def _scene(seed=21, crowns=36):
    """A four-band uint8 RGBI image with blob crowns (bright or dark in the near-infrared band), an nDSM on a 1 m grid with their
    heights, and the crowns' rings with falling scores; every third crown once more, shifted by two pixels with a lower score (a
    duplicate for the IoU filter), and a crown of half the radius inside every fourth (nested, for containment)."""
    rng = np.random.default_rng(seed)
    rgbi = rng.integers(40, 120, (4, SIDE, SIDE), dtype=np.uint8)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    fine = rng.uniform(0, 1.0, (SIDE, SIDE)).astype(np.float32)
    rings, scores = [], []
    for k in range(crowns):
        cx, cy, r = rng.uniform(40, SIDE - 40), rng.uniform(40, SIDE - 40), rng.uniform(16, 28)
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        inside = d2 < r ** 2
        rgbi[3][inside] = 220 if k % 4 else 60
        hgt = float(rng.uniform(1.2, 2.2) if k % 5 == 0 else rng.uniform(5.0, 25.0))
        fine[inside] = np.maximum(fine[inside], hgt * (1 - d2[inside] / r ** 2 * 0.5))
        rings.append(_ring(cx, cy, r))
        scores.append(0.97 - 0.015 * k)
        if k % 3 == 0:
            rings.append(_ring(cx + 2, cy, r))
            scores.append(0.5 - 0.005 * k)
        if k % 4 == 1:
            rings.append(_ring(cx, cy, 0.5 * r))
            scores.append(0.6 - 0.005 * k)
    ndsm = fine.reshape(SIDE // 5, 5, SIDE // 5, 5).max(axis=(1, 3)).astype(np.float32)
    return rgbi, ndsm, rings, scores


def _config(device_filters, area_threshold=1):
    cfg = {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": area_threshold, "containment_threshold": 0.9, "height_threshold": 3.0,
           "ndvi_mean_threshold": 0.2, "ndvi_var_threshold": 0.5, "use_overlap": False, "tile_width": 50, "tile_height": 50, "buffer": 10,
           "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": 0.2, "height_scaling_factor": 1.0,
           "device_decode": False}
    if device_filters is not None:
        cfg["device_filters"] = device_filters
    return cfg


def _same_features(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


@pytest.fixture
def filters(monkeypatch):
    """Records what the four filter functions are given and return while process_layer runs."""
    seen = []
    for name in ("filter_polygons_by_iou_and_area", "filter_polygons_by_iou_and_area_device", "containment", "containment_device"):
        def recording(*args, _real=getattr(P, name), _name=name, **kw):
            out = _real(*args, **kw)
            seen.append((_name, len(args[0]), out))
            return out
        monkeypatch.setattr(P, name, recording)
    return seen


@pytest.fixture
def rasters(tmp_path):
    rgbi, ndsm, rings, scores = _scene()
    rpath, hpath = str(tmp_path / "rgbi.tif"), str(tmp_path / "ndsm.tif")
    write_geotiff(rpath, rgbi, T, 25832, compression="deflate", tile=(128, 128))
    write_geotiff(hpath, ndsm[None], NT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    return rings, scores, hpath, rpath


def test_process_layer_is_the_same_on_both_paths(rasters, filters, capsys):
    rings, scores, hpath, rpath = rasters
    host = P.process_layer(rings, scores, _config(False), hpath, rpath)
    assert [s[0] for s in filters] == ["filter_polygons_by_iou_and_area", "containment"]
    (_, n_in, kept), (_, n_kept, (_, is_c, num)) = filters
    assert len(kept) == n_kept < n_in                       # the IoU filter removes the duplicates ...
    assert any(is_c) and {1} <= set(num)                    # ... and containment finds the nested crowns
    assert 0 < len(host) < n_kept
    del filters[:]
    dev = P.process_layer(rings, scores, _config(True), hpath, rpath)
    assert [s[0] for s in filters] == ["filter_polygons_by_iou_and_area_device", "containment_device"]      # neither declined
    assert filters[0][2] == kept and filters[1][2] == ([1.0] * n_kept, is_c, num)
    assert "using the host function" not in capsys.readouterr().out
    _same_features(host, dev)
    for cfg in (_config("auto"), _config(None)):            # "auto" and an absent key keep the host functions
        del filters[:]
        _same_features(host, P.process_layer(rings, scores, cfg, hpath, rpath))
        assert [s[0] for s in filters] == ["filter_polygons_by_iou_and_area", "containment"]


def test_a_degenerate_ring_sends_both_filters_back_to_the_host(rasters, filters, capsys):
    """A ring without extent in y (a box of area 0, let through by ``area_threshold: 0``): both device wrappers decline, one printed
    line each, and the features are the host path's."""
    rings, scores, hpath, rpath = rasters
    flat = np.array([[412030.0, 5318060.0], [412040.0, 5318060.0], [412050.0, 5318060.0], [412030.0, 5318060.0]])
    rings, scores = rings + [flat], scores + [0.9]
    host = P.process_layer(rings, scores, _config(False, area_threshold=0), hpath, rpath)
    capsys.readouterr()
    del filters[:]
    dev = P.process_layer(rings, scores, _config(True, area_threshold=0), hpath, rpath)
    assert [(s[0], s[2] is None) for s in filters] == [("filter_polygons_by_iou_and_area_device", True), ("filter_polygons_by_iou_and_area", False),
                                                       ("containment_device", True), ("containment", False)]
    out = capsys.readouterr().out
    assert out.count("using the host function") == 2 and out.count("no finite positive float32 area") == 2
    assert len(host) > 0
    _same_features(host, dev)
