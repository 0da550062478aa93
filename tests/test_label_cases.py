"""td_crown_labels, the host twin of the label kernel, through crown_label_raster(device=None): equal to the expectation of
label_cases.py — the exact oracle's pixel sets composited by the unsigned maximum in numpy — pixel for pixel and status for status
on every case of every family of zonal_cases.FAMILIES and on every overlap case; and controls that the checker reports what it
should, and that crown_priorities is the order it says."""
import numpy as np
import pytest

from treedetection_amd import postprocessing as P

import label_cases as L
import zonal_cases as Z


def _host(case):
    labels = L.before(case)
    got, status = P.crown_label_raster(list(case.rings), case.values, case.transform, case.shape, device=None, out=labels)
    assert got is labels
    return got, status


def test_every_family_and_every_overlap_case_is_listed():
    names = [c.name for c in L.label_cases()]
    assert len(names) == len(set(names))
    for family in Z.FAMILIES:
        assert sum(n.startswith(family + "/") for n in names) == len(Z.cases(family)) > 0
    for extra in ("crossing_high_first", "crossing_high_last", "equal", "zero_between", "sign_bit_0", "sign_bit_1", "sign_bit_2", "many_waves",
                  "prefilled"):
        assert extra in names
    many = next(c for c in L.label_cases() if c.name == "many_waves")
    assert len(many.rings) > Z.IN_FLIGHT and np.unique(many.values[:-1]).size == len(many.rings) - 1
    pre = next(c for c in L.label_cases() if c.name == "prefilled")
    inside = L.composite(pre.shape, pre.pixels, np.ones(3, np.uint32), [0]) == 1          # ring 0, value 5000
    assert (pre.before[inside] > 5000).any() and (pre.before[inside] < 5000).any()
    assert all(max(c.shape) <= 140 for c in L.label_cases())


def test_the_host_twin_equals_the_expected_raster_on_every_case():
    reports = []
    for case in L.label_cases():
        want = L.expected(case)
        got = _host(case)
        covered = int((want[0] != L.before(case)).sum())
        print(f"{case.name}: {len(case.rings)} rings on {case.shape}, {covered} pixels change, statuses {np.bincount(want[1], minlength=3).tolist()}")
        reports.append(L.report(case, got, want))
    assert not any(reports), "\n".join(r for r in reports if r)


def test_default_raster_is_zeroed_and_values_are_checked():
    case = next(c for c in L.label_cases() if c.name == "crossing_high_first")
    labels, status = P.crown_label_raster(list(case.rings), [9, 4], case.transform, case.shape, device=None)
    assert L.report(case, (labels, status), L.expected(case)) is None
    for bad in ([9.0, 4.0], [9, -1], [9, 1 << 32], [9], [True, False], [[9, 4]]):
        with pytest.raises(ValueError, match="unsigned integers below 2\\^32"):
            P.crown_label_raster(list(case.rings), bad, case.transform, case.shape, device=None)
    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels"):
        P.crown_label_raster(list(case.rings), [9, 4], case.transform, (0, 5), device=None)
    empty, st = P.crown_label_raster([], [], case.transform, (3, 4), device=None)
    assert empty.shape == (3, 4) and empty.dtype == np.uint32 and not empty.any() and st.shape == (0,)


# ---- controls ------------------------------------------------------------------------------------------------------------------
def test_control_one_altered_pixel_is_reported():
    case = next(c for c in L.label_cases() if c.name == "sign_bit_1")
    got = _host(case)
    want_labels, want_status = L.expected(case)
    assert L.report(case, got, (want_labels, want_status)) is None
    for r, c in ((0, 0), case.pixels[0][0], case.pixels[2][-1]):
        altered = want_labels.copy()
        altered[r, c] ^= 1
        msg = L.report(case, got, (altered, want_status))
        assert msg and "1 of 900 pixels differ" in msg and f"({r}, {c})" in msg
    status = want_status.copy()
    status[1] = 2
    assert "1 statuses differ" in L.report(case, got, (want_labels, status))


def test_control_a_minimum_composite_is_reported():
    for name in ("crossing_high_first", "crossing_high_last", "sign_bit_0", "sign_bit_2", "many_waves"):
        case = next(c for c in L.label_cases() if c.name == name)
        drawn = range(len(case.rings))
        low = L.composite(case.shape, case.pixels, case.values, drawn, np.full(case.shape, 0xFFFFFFFF, np.uint32), rule=np.minimum)
        low[L.composite(case.shape, case.pixels, np.ones(len(case.rings), np.uint32), drawn) == 0] = 0       # pixels no ring covers
        assert L.report(case, _host(case), (low, L.expected(case)[1])) is not None, name
    # and a signed maximum on the sign-bit values
    case = next(c for c in L.label_cases() if c.name == "sign_bit_0")
    signed = L.composite(case.shape, case.pixels, case.values, range(3), rule=lambda a, v: np.maximum(a.view(np.int32), v.view(np.int32)).view(np.uint32))
    assert L.report(case, _host(case), (signed, L.expected(case)[1])) is not None


def test_priorities_follow_a_sort_written_out():
    rng = np.random.default_rng(7)
    for scores in ([0.5], [0.9, 0.8, 0.9, 0.1, 0.8, 0.9], list(rng.integers(0, 5, 200) / 4.0), list(rng.random(50)), [0.0, -0.0, float("inf"), 0.0]):
        n = len(scores)
        priority, table = P.crown_priorities(scores)
        assert priority.dtype == np.uint32 and table.dtype == np.uint32 and table.shape == (n + 1,)
        assert sorted(priority.tolist()) == list(range(1, n + 1))
        for i in range(n):                                    # i beats j: the higher score, or the same score and the lower index
            for j in range(n):
                if i != j:
                    wins = scores[i] > scores[j] or (scores[i] == scores[j] and i < j)
                    assert (priority[i] > priority[j]) == wins, (scores[i], scores[j], i, j)
        assert table[0] == 0 and [int(table[p]) for p in priority] == list(range(1, n + 1))
        raster = np.concatenate([[0], priority, priority[::-1]]).astype(np.uint32).reshape(1, -1)
        assert P.labels_from_priorities(raster, table).tolist() == [[0, *range(1, n + 1), *range(n, 0, -1)]]
    _, table = P.crown_priorities([0.3, 0.7], labels=[40, 50])
    assert table.tolist() == [0, 40, 50]
    p, table = P.crown_priorities([])
    assert p.shape == (0,) and table.tolist() == [0]
    for bad in ([0.5, float("nan")], [float("nan")]):
        with pytest.raises(ValueError, match="NaN"):
            P.crown_priorities(bad)


def test_the_setting_refuses_what_it_does_not_know():
    assert P.crown_rasters_setting() is False and P.crown_rasters_setting(None) is False and P.crown_rasters_setting(False) is False
    assert P.crown_rasters_setting("height") == "height" and P.crown_rasters_setting("image") == "image"
    for bad in (True, "both", 1, "Height", ["height"]):
        with pytest.raises(ValueError, match="crown_rasters must be false, 'height' or 'image'"):
            P.crown_rasters_setting(bad)
