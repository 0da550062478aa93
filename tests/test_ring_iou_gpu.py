"""td_ring_pairs_area_dev (ringiou.hip: a wave per ring pair) against its host twin td_ring_pairs_area — the same header, the
wave's lanes emulated — BIT FOR BIT (inter and both areas), at the smallest shapes where the kernel can go wrong; clean_crowns and
candidate_pairs on the device against the host path. The host twin is held to the exact oracle in tests/test_ring_iou.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_iou_ref as R  # noqa: E402
from treedetection_amd import _lib  # noqa: E402
from treedetection_amd import cleaning as CL  # noqa: E402
from treedetection_amd import gpkg  # noqa: E402
from treedetection_amd import postprocessing as P  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, WPB, GRID = _lib.RING_PAIR_CAP, _lib.RING_PAIR_WPB, _lib.RING_PAIR_GRID


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def both(rings_a, rings_b, pairs, host_for_capped=False):
    """(device out, device status, host out, host status) of one pair list."""
    xa, sa = CL.pack_rings(rings_a)
    xb, sb = (xa, sa) if rings_b is rings_a else CL.pack_rings(rings_b)
    d_out, d_st = CL.ring_pairs_area_packed(xa, sa, xb, sb, pairs, 0, host_for_capped=host_for_capped)
    h_out, h_st = CL.ring_pairs_area_packed(xa, sa, xb, sb, pairs, None)
    return d_out, d_st, h_out, h_st


def test_term_counts_around_a_wave_and_every_case_family_two_ring_sets():
    """m x n in {3x3, 7x9 = 63, 8x8 = 64, 5x13 = 65, 3x43 = 129, 3x4, 4x4} and the oracle's case families (convex, star, nested,
    shared edges, twins, grid-snapped, both windings, UTM, slivers), set A != set B, in one launch."""
    all_cases = R.wave_cases() + R.cases()
    ring_a, ring_b = [c[1] for c in all_cases], [c[2] for c in all_cases]
    pairs = [[k, k] for k in range(len(all_cases))] + [[0, 5], [5, 0], [3, 3], [3, 3]]        # cross pairs and a repeated pair
    d_out, d_st, h_out, h_st = both(ring_a, ring_b, pairs)
    assert (d_st == 0).all() and (h_st == 0).all()
    for k, (i, j) in enumerate(pairs):
        assert np.array_equal(bits(d_out[k]), bits(h_out[k])), (all_cases[i][0], all_cases[j][0], d_out[k], h_out[k])
    assert (d_out[:, 0] >= 0).all() and not np.signbit(d_out[:, 0]).any()


def test_self_pairs_and_one_ring_set_on_both_sides():
    rings = [c[1] for c in R.cases()[:8]]
    pairs = [[k, k] for k in range(8)] + [[0, 1], [1, 0], [2, 7]]
    d_out, d_st, h_out, _ = both(rings, rings, pairs)
    assert (d_st == 0).all() and np.array_equal(bits(d_out), bits(h_out))
    assert np.allclose(d_out[:8, 0], d_out[:8, 1], rtol=1e-13, atol=0)              # a ring with itself: its own area


def test_the_lds_cap_and_one_vertex_past_it():
    tri = np.array([[0.5, -1.0], [2.5, 0.25], [-1.0, 2.0]])
    at_cap, past_cap = R.regular(CAP - 3, r=3.0), R.regular(CAP - 2, r=3.0)
    half = R.regular(CAP // 2, r=3.0), R.regular(CAP // 2, centre=(0.7, -0.4), r=2.5, phase=0.3)      # the most terms a wave takes
    ring_a, ring_b = [at_cap, past_cap, half[0], tri], [tri, half[1], past_cap]
    pairs = [[0, 0], [1, 0], [2, 1], [3, 2], [3, 0]]
    d_out, d_st, h_out, h_st = both(ring_a, ring_b, pairs)
    assert d_st.tolist() == [0, 1, 0, 1, 0] and (h_st == 0).all()
    assert np.isnan(d_out[[1, 3]]).all()
    assert np.array_equal(bits(d_out[[0, 2, 4]]), bits(h_out[[0, 2, 4]]))
    w_out, w_st, _, _ = both(ring_a, ring_b, pairs, host_for_capped=True)          # the wrapper serves the capped pairs from the host
    assert w_st.tolist() == [0, 1, 0, 1, 0] and np.array_equal(bits(w_out), bits(h_out))
    iou, areas = CL.ring_pairs_iou(ring_a, ring_b, pairs, 0)
    assert np.array_equal(bits(areas), bits(h_out)) and np.array_equal(bits(iou), bits(CL.iou_of(h_out)))


@pytest.mark.parametrize("count", [1, WPB - 1, WPB, WPB + 1, GRID * WPB + 1])
def test_pair_counts_around_a_workgroup_and_past_the_grid(count):
    """One pair, waves-per-workgroup +- 1, and one pair more than the grid's waves hold: the grid-stride loop runs."""
    rings = [c[1] for c in R.wave_cases()] + [c[2] for c in R.wave_cases()]
    if count > 100:
        rings = [r for r in rings if len(r) <= 9]            # (the host twin computes them all too: keep the terms few)
    rng = np.random.default_rng(count)
    pairs = rng.integers(0, len(rings), (count, 2)).astype(np.int32)
    d_out, d_st, h_out, h_st = both(rings, rings, pairs)
    assert (d_st == 0).all() and (h_st == 0).all() and np.array_equal(bits(d_out), bits(h_out))


def test_no_pairs_is_no_launch():
    import torch
    lib = _lib.load()
    buf = torch.zeros(16, dtype=torch.float64, device="cuda")
    start = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    out = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    args = [buf.data_ptr(), start.data_ptr(), 1, buf.data_ptr(), start.data_ptr(), 1, pairs.data_ptr(), 0, out.data_ptr(), status.data_ptr(),
            _lib.stream_ptr()]
    assert lib.td_ring_pairs_area_dev(*args) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0, 7.0] and status.tolist() == [9]
    # refused before any launch: null pointers, a negative count, a misaligned vertex array
    for k in (0, 1, 3, 4, 6, 8, 9):
        a = list(args)
        a[k], a[7] = None, 1
        assert lib.td_ring_pairs_area_dev(*a) == _lib.ERR_INVALID and b"null" in lib.td_last_error()
    a = list(args)
    a[7] = -1
    assert lib.td_ring_pairs_area_dev(*a) == _lib.ERR_INVALID and b"n_pairs" in lib.td_last_error()
    a = list(args)
    a[0], a[7] = buf.data_ptr() + 8, 1
    assert lib.td_ring_pairs_area_dev(*a) == _lib.ERR_INVALID and b"aligned" in lib.td_last_error()
    out_h, st_h = CL.ring_pairs_area_packed(np.zeros((4, 2)), [0, 4], np.zeros((4, 2)), [0, 4], np.zeros((0, 2), np.int32), 0)
    assert out_h.shape == (0, 3) and st_h.shape == (0,)


def test_refused_pairs_get_status_2_and_nan_and_the_rest_of_the_launch_is_served():
    """An index outside its ring set, a 2-vertex ring and a non-finite coordinate are refused INPUTS: status 2, NaN, the kernel
    touches no ring memory for them; the valid pairs of the same launch come out as ever."""
    good = [c[1] for c in R.wave_cases()]
    nan_ring, inf_ring = good[1].copy(), good[2].copy()
    nan_ring[3, 1] = np.nan
    inf_ring[0, 0] = -np.inf
    ring_a = good + [np.array([[0, 0], [1, 1.0]]), nan_ring, inf_ring, np.zeros((0, 2))]
    n = len(ring_a)
    two, nan_i, inf_i, empty = n - 4, n - 3, n - 2, n - 1
    pairs = [[0, 1], [n, 0], [0, n], [-1, 0], [0, -1], [2 ** 31 - 1, 0], [-2 ** 31, 1], [two, 0], [0, two], [nan_i, 0], [0, inf_i], [empty, 0], [1, 2]]
    d_out, d_st, h_out, h_st = both(ring_a, ring_a, pairs)
    assert d_st.tolist() == [0] + [2] * 11 + [0] and h_st.tolist() == d_st.tolist()
    assert np.isnan(d_out[1:12]).all() and np.array_equal(bits(d_out[[0, 12]]), bits(h_out[[0, 12]]))
    with pytest.raises(ValueError, match="refused"):
        CL.ring_pairs_iou(ring_a, ring_a, [[0, 1], [two, 0]], 0)
    with pytest.raises(ValueError, match="refused"):
        CL.ring_pairs_iou(ring_a, ring_a, [[n, 0]], 0)


@pytest.mark.parametrize("n", [1, 2, 257, 1025])
def test_clean_crowns_on_the_device_equals_the_host_path(n):
    """The scenes of tests/test_clean_crowns.py at the candidate kernels' row block (256) and column chunk (1 024), plus one."""
    rings, scores = R.crown_scene(n, 2)
    for kw in ({}, {"iou_threshold": 0.5, "confidence": 0, "area_threshold": 0}):
        want = CL.clean_crowns(rings, scores, device=None, **kw)
        assert CL.clean_crowns(rings, scores, device=0, **kw) == want
    if n >= 257:
        assert 0 < len(want) < n
        boxes = np.array([[r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()] for r in rings])
        host_pairs = {tuple(p) for p in CL.candidate_pairs_host(boxes).tolist()}
        dev_pairs = {tuple(p) for p in CL.candidate_pairs(boxes, 0).tolist()}
        assert host_pairs <= dev_pairs and len(dev_pairs) <= len(host_pairs) + n and all(i < j for i, j in dev_pairs)


def test_candidate_pairs_keeps_a_pair_that_plain_float32_rounding_loses():
    """UTM coordinates, a layer 5 km wide: two boxes that overlap by 5e-8 in x. Relative to the layer's corner both edges round to
    the same float32 — a plain cast loses the pair; rounded outward it stays."""
    x0, y0 = 412000.0, 5318000.0
    boxes = np.array([[x0, y0, x0 + 10, y0 + 10],                               # the layer's lower-left corner
                      [x0 + 4090, y0 + 100, x0 + 4096.0000001, y0 + 110],
                      [x0 + 4096.00000005, y0 + 105, x0 + 4100, y0 + 112],
                      [x0 + 4990, y0 + 4000, x0 + 5000, y0 + 4010],
                      [x0 + 4096.5, y0 + 105, x0 + 4100, y0 + 112]])            # overlaps box 2 only
    assert boxes[1, 2] > boxes[2, 0]                                            # float64: a positive overlap
    exact = [(i, j) for i in range(5) for j in range(i + 1, 5)
             if min(boxes[i, 2], boxes[j, 2]) > max(boxes[i, 0], boxes[j, 0]) and min(boxes[i, 3], boxes[j, 3]) > max(boxes[i, 1], boxes[j, 1])]
    assert exact == [(1, 2), (2, 4)]
    rel = (boxes - np.tile(boxes[:, :2].min(axis=0) - 1.0, 2)).astype(np.float32)
    assert rel[1, 2] == rel[2, 0], "the plain float32 cast must lose the pair for this test to mean anything"
    got = [tuple(p) for p in CL.candidate_pairs(boxes, 0).tolist()]
    assert set(exact) <= set(got) and [tuple(p) for p in CL.candidate_pairs_host(boxes).tolist()] == exact
    # what the device path declines goes to the host sweep, same pairs
    wide = boxes.copy()
    wide[3, 2] += 2.0 ** 25
    assert [tuple(p) for p in CL.candidate_pairs(wide, 0).tolist()] == exact


def test_config_key_through_the_real_crown_stage(tmp_path):
    """process_single_file on rasters: ``clean_crowns: false`` writes what a run without the key writes; ``true`` writes what the
    stage writes for the layer thinned by clean_crowns(iou_threshold=0.7, confidence=0, area_threshold=0)."""
    import re
    import sqlite3
    from test_postprocessing import _scene

    os.makedirs(tmp_path / "img")
    os.makedirs(tmp_path / "ndsm")
    rng = np.random.default_rng(9)
    _, _, _, _, crowns, _ = _scene(tmp_path, rng, same_grid=False)
    scores = [0.95 - 0.03 * k for k in range(len(crowns))]
    c = crowns[0].mean(axis=0)
    crowns.append(c + (crowns[0] - c) * 0.93)                   # outline IoU 0.86 with crown 0, lower score
    scores.append(0.5)
    src = str(tmp_path / "3241.gpkg")
    gpkg.write_polygons(src, crowns, {"Confidence_score": scores}, 25832)
    base = {"confidence_threshold": 0.3, "iou_threshold": 0.99, "area_threshold": 1, "containment_threshold": 0.99, "height_threshold": 0,
            "use_overlap": False, "ndvi_scaling_factor": 1.0, "height_scaling_factor": 1.0}

    def run(name, layer, extra):
        out = str(tmp_path / name / "processed_3241.gpkg")
        os.makedirs(tmp_path / name)
        assert P.process_single_file(layer, out, str(tmp_path / "ndsm" / "3241.tif"), str(tmp_path / "img" / "3241.tif"), device_id="0",
                                     config=dict(base, **extra)) == layer
        con = sqlite3.connect(out)
        try:
            return [re.sub(r"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.\d+Z", "<now>", line) for line in con.iterdump()]
        finally:
            con.close()

    absent, false, true = run("absent", src, {}), run("false", src, {"clean_crowns": False}), run("true", src, {"clean_crowns": True})
    assert false == absent
    kept = CL.clean_crowns(crowns, scores, iou_threshold=0.7, confidence=0, area_threshold=0, device=0)
    assert kept == list(range(len(crowns) - 1))                 # the near-duplicate goes, nothing else
    thinned = str(tmp_path / "thin" / "3241.gpkg")
    os.makedirs(tmp_path / "thin")
    gpkg.write_polygons(thinned, [crowns[k] for k in kept], {"Confidence_score": [scores[k] for k in kept]}, 25832)
    assert true == run("want", thinned, {}) and true != absent
