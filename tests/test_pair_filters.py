"""The host side of the crown stage's device filters (``device_filters: true``): the greedy pass over sparse rows
(td_crown_pairs_greedy) against oracle.postprocess_ref.filter_by_iou_and_area on the case families of pair_cases.py, the
preconditions under which the two device wrappers hand the work back to the host functions, and the configuration key. No GPU."""
import numpy as np
import pytest

from oracle import postprocess_ref as O
from treedetection_amd import box_pairs as BP
from treedetection_amd import postprocessing as P

import pair_cases


def _csr(mask, keep_diagonal=False, rng=None):
    """Sparse rows of an N x N mask (the diagonal left out, as the kernels leave it out), optionally shuffled inside each row."""
    m = mask.copy()
    if not keep_diagonal:
        np.fill_diagonal(m, False)
    rows = [np.flatnonzero(r) for r in m]
    if rng is not None:
        rows = [rng.permutation(r) for r in rows]
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return row_start, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


def _kept(case, **kw):
    mask = pair_cases.oracle_mask(case)
    removed = P.greedy_removal(*_csr(mask, **kw), np.array(case.scores, dtype=np.float16), mask.diagonal().copy())
    return [int(i) for i in np.flatnonzero(~removed)]


@pytest.mark.parametrize("n", [1, 2, 97, 600])
@pytest.mark.parametrize("family", pair_cases.FAMILIES)
def test_greedy_pass_over_sparse_rows_keeps_what_the_oracle_keeps(family, n):
    case = pair_cases.make(family, n, seed=3)
    want = O.filter_by_iou_and_area(case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold)
    assert _kept(case) == want
    assert _kept(case, rng=np.random.default_rng(n)) == want                       # the order inside a row does not matter
    assert _kept(case, keep_diagonal=True, rng=np.random.default_rng(n + 1)) == want   # nor does a row that lists itself
    assert P.filter_polygons_by_iou_and_area(case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold) == want


def test_the_case_families_exercise_what_they_are_for():
    """The crafted inputs do what pair_cases.py says, judged on the oracle alone: groups with several members, a removed crown that
    is the best of a later group, float16 ties, an unset diagonal on a connected row, both exact thresholds, 0 .. 3+ contained."""
    n = 600
    masks = {f: pair_cases.oracle_mask(pair_cases.make(f, n, seed=3)) for f in pair_cases.FAMILIES}
    off = {f: m & ~np.eye(n, dtype=bool) for f, m in masks.items()}
    assert off["a"].any() and (off["b"].sum(axis=1) >= 3).any()
    for f in pair_cases.FAMILIES:
        case = pair_cases.make(f, n, seed=3)
        kept = O.filter_by_iou_and_area(case.bounds, case.areas, case.scores, case.iou_threshold, case.area_threshold)
        assert 0 < len(kept) < n, f
    # c: a row whose best member was removed by an earlier row
    case = pair_cases.make("c", n, seed=3)
    conf = np.array(case.scores, dtype=np.float16)
    removed, hit = np.zeros(n, bool), False
    for i in range(n):
        if removed[i]:
            continue
        members = np.append(np.where(masks["c"][i])[0], i)
        best = members[int(np.argmax(conf[members]))]
        hit |= bool(removed[best])
        removed[[j for j in members if j != best]] = True
    assert hit
    # d: equal float16 scores that differ in float64 inside one group, and a connected row whose diagonal is unset
    case = pair_cases.make("d", n, seed=3)
    conf = np.array(case.scores, dtype=np.float16)
    i, j = np.nonzero(off["d"])
    assert ((conf[i] == conf[j]) & (np.array(case.scores)[i] != np.array(case.scores)[j])).any()
    assert (~masks["d"].diagonal() & off["d"].any(axis=1)).any()
    # e: the pair at IoU 0.5 is not connected; the pair at ratio 0.5 is contained
    case = pair_cases.make("e", 6, seed=3)
    assert case.bounds[:2] == [(0.0, 0.0, 2.0, 2.0), (0.0, 0.0, 2.0, 1.0)]
    m6 = pair_cases.oracle_mask(case)
    assert not m6[0, 1] and m6[4, 5]
    ratios, is_c, num = O.containment(case.bounds, case.containment_threshold)
    assert num[2] == 1 and is_c[3] and O.box_iou(np.array(case.bounds[:2], np.float32), np.array(case.bounds[:2], np.float32))[0, 1] == 0.5
    # f: every count from 0 to 3 and beyond
    case = pair_cases.make("f", n, seed=3)
    _, is_c, num = O.containment(case.bounds, case.containment_threshold)
    assert {0, 1, 2, 3} <= set(num) and max(num) > 3 and any(is_c) and not all(is_c)


def test_greedy_pass_refuses_malformed_rows():
    conf = np.array([0.5, 0.6, 0.7], np.float16)
    for row_start, cols in (([0, 1, 1, 3], [1, 0, 3]), ([0, 2, 1, 2], [1, 2]), ([1, 1, 1, 1], [])):
        with pytest.raises(Exception, match="td_crown_pairs_greedy|greedy_removal"):
            P.greedy_removal(np.array(row_start, np.int64), np.array(cols, np.int32), conf)
    assert not P.greedy_removal(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float16)).size


BOX = [(412000.0, 5318000.0, 412004.0, 5318004.0), (412001.0, 5318001.0, 412003.0, 5318003.0)]


@pytest.fixture
def no_device(monkeypatch):
    """The wrappers decide on the host, before anything touches the GPU library."""
    def fail(*a, **k):
        raise AssertionError("the device path was entered")
    monkeypatch.setattr(BP, "connected_pairs_device", fail)
    monkeypatch.setattr(BP._lib, "load", fail)
    monkeypatch.setattr(BP._lib, "stream_ptr", fail)


@pytest.mark.parametrize("what, bounds, confidences, iou_threshold", [
    ("coordinate", [BOX[0], (412001.0, float("inf"), 412003.0, 5318003.0)], [0.9, 0.8], 0.5),
    ("coordinate", [BOX[0], (float("nan"), 5318001.0, 412003.0, 5318003.0)], [0.9, 0.8], 0.5),
    ("area", [BOX[0], (412001.0, 5318001.0, 412001.0, 5318003.0)], [0.9, 0.8], 0.5),          # zero width
    ("area", [BOX[0], (412001.0, 5318001.1, 412003.0, 5318001.2)], [0.9, 0.8], 0.5),          # zero height in float32 only
    ("area", [BOX[0], (412003.0, 5318001.0, 412001.0, 5318003.0)], [0.9, 0.8], 0.5),          # negative
    ("area", [BOX[0], (-3e38, -3e38, 3e38, 3e38)], [0.9, 0.8], 0.5),                          # overflows
    ("NaN", BOX, [0.9, float("nan")], 0.5),
    ("negative", BOX, [0.9, 0.8], -0.1),
    ("float32", BOX, [0.9, 0.8], np.float64(0.5)),
])
def test_dedup_wrapper_hands_back_what_the_kernels_were_not_argued_for(no_device, capsys, what, bounds, confidences, iou_threshold):
    assert P.filter_polygons_by_iou_and_area_device(bounds, [12.0, 4.0], confidences, iou_threshold, 3) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and what in out and "using the host function" in out


@pytest.mark.parametrize("what, bounds, threshold", [
    ("coordinate", [BOX[0], (412001.0, float("-inf"), 412003.0, 5318003.0)], 0.9),
    ("area", [BOX[0], (412001.0, 5318001.1, 412003.0, 5318001.2)], 0.9),
    ("positive", BOX, 0.0),
    ("positive", BOX, -0.5),
    ("float32", BOX, np.float64(0.9)),
])
def test_containment_wrapper_hands_back_what_the_kernels_were_not_argued_for(no_device, capsys, what, bounds, threshold):
    assert P.containment_device(bounds, threshold) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and what in out and "using the host function" in out


def test_empty_input_returns_what_the_host_functions_return(no_device):
    assert P.filter_polygons_by_iou_and_area_device([], [], [], 0.5, 3) == P.filter_polygons_by_iou_and_area([], [], [], 0.5, 3) == []
    assert P.containment_device([], 0.9) == P.containment([], 0.9) == ([], [], [])


def test_too_many_connected_pairs_hand_back(monkeypatch, capsys):
    monkeypatch.setattr(BP, "connected_pairs_device", lambda *a, **k: None)       # what it returns above MAX_DEVICE_PAIRS
    assert P.filter_polygons_by_iou_and_area_device(BOX, [12.0, 4.0], [0.9, 0.8], 0.5, 3) is None
    assert f"more than {1 << 27} connected pairs" in capsys.readouterr().out


def test_device_filters_key_is_read_strictly():
    for value, on in ((True, True), ("true", True), (False, False), ("false", False), ("auto", False), (None, False)):
        assert P._device_filters_on({"device_filters": value}) is on
    assert P._device_filters_on({}) is False
    for bad in ("sometimes", 1, 0, "yes", "all"):
        with pytest.raises(ValueError, match="device_filters"):
            P._device_filters_on({"device_filters": bad})
    with pytest.raises(ValueError, match="device_filters must be true, false or 'auto', got 'sometimes'"):
        P.process_layer([], [], {"device_filters": "sometimes"}, "no-height.tif", "no-rgbi.tif")
