"""td_crown_zonal (crownzonal_host.cpp), the host twin of the zonal kernel, against the exact oracle of zonal_cases.py on every
family; the facts the cases state, checked with the oracle alone; the ``crown_statistics`` setting and the resume parameters. No GPU.

Contract (zonal_cases.differing): status, count, minimum, maximum and the position of the maximum equal the oracle bit for bit (a
NaN's payload aside); mean and variance lie within one float32 ulp of the oracle's exact rational rounded once. The bound is derived,
not tuned: any order of N float64 additions errs by at most (N - 1) * 2^-53 * sum|v|; with N <= 2^15 pixels per crafted crown that
is below 2^-38 * sum|v|. Every moment case has values of one sign (sum|v| = |sum v|) and a spread of at least 2^-10 of the mean, so
the float64 mean and variance are within 2^-37 relatively of the exact ones — far under half a float32 ulp — and their float32
rounding is the once-rounded value or its neighbour. The constant case is exact (zonal_cases.moment_differs spells the steps out)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P

import zonal_cases as Z


def _host(case):
    return P.crown_zonal_stats(np.array(case.raster), case.transform, Z.launch_rings(case), device=None)


def _report(case, got, want):
    bad = np.flatnonzero(Z.differing(got, want))
    if not bad.size:
        return None
    k = int(bad[0])
    return (f"{case.name}: {bad.size} of {want.status.size} crowns differ, first crown {k}: got status {got[3][k]} count {got[1][k]} pos "
            f"{got[2][k].tolist()} stats {got[0][k].tolist()}, want status {want.status[k]} count {want.count[k]} pos {want.pos[k].tolist()} "
            f"stats {want.stats[k].tolist()}")


def test_the_capacity_the_cases_assume_is_the_librarys():
    assert Z.RING_CAP == _lib.ZONAL_RING_CAP >= 256
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "treedet.h")).read()
    assert f"#define TD_ZONAL_RING_CAP {Z.RING_CAP} " in header


@pytest.mark.parametrize("family", list(Z.FAMILIES))
def test_host_twin_equals_the_oracle(family):
    report = []
    for i, case in enumerate(Z.cases(family)):
        want = Z.expected(family, i)
        got = _host(case)
        print(f"{family} {case.name}: {want.status.size} crowns, counts {want.count[:12].tolist()}")
        report.append(_report(case, got, want))
        stats, count, pos, status = got
        assert (status[want.status == 2] == 2).all() and (status != 1).all()          # the host function has no capacity
        refused = status == 2
        assert np.isnan(stats[refused]).all() and (count[refused] == -1).all() and (pos[refused] == -1).all()
        empty = (status == 0) & (count == 0)
        assert (stats[empty] == -1.0).all() and (pos[empty] == -1).all()
        if "constant" in case.facts:                                  # known answer, exact: min = max = mean = the value, variance 0
            v = np.float32(case.facts["constant"])
            assert np.array_equal(Z._bits(stats), Z._bits(np.tile(np.array([v, v, v, 0.0], np.float32), (stats.shape[0], 1))))
        for group in case.facts.get("groups", []):                    # one ring, reversed / rotated / repeated: identical rows
            for j in group[1:]:
                assert np.array_equal(Z._bits(stats[group[0]]), Z._bits(stats[j])) and count[group[0]] == count[j] and (pos[group[0]] == pos[j]).all()
    assert not any(report), "\n".join(r for r in report if r)


def test_the_facts_the_cases_state_hold_in_the_oracle():
    """Counts worked out by hand, pixels that must be outside, rows that must be empty, what each value family aims at — all
    against the oracle, none against the library."""
    for family in Z.FAMILIES:
        for i, case in enumerate(Z.cases(family)):
            want, pix = Z.expected(family, i), Z.inside(family, i)
            counts = case.facts.get("counts", [])
            for k, c in (counts.items() if isinstance(counts, dict) else enumerate(counts)):
                assert c is None or want.count[k] == c, (case.name, k, c, want.count[k])
            for k in case.facts.get("empty", []):
                assert want.status[k] == 0 and want.count[k] == 0 and (want.stats[k] == -1).all() and (want.pos[k] == -1).all()
            for k, notch in case.facts.get("notches", {}).items():
                ring = case.rings[k]
                for r, c in notch:                                    # in the box, outside the ring; the raster's largest value
                    X, Y = Z.centres(case.transform, *case.raster.shape)
                    assert ring[:, 0].min() < X[r, c] < ring[:, 0].max() and ring[:, 1].min() < Y[r, c] < ring[:, 1].max()
                    assert (r, c) not in pix[k] and case.raster[r, c] == case.raster.max()
                assert want.stats[k, 1] < case.raster.max()
            for k, (r, c) in case.facts.get("outside", {}).items():
                assert (r, c) not in pix[k]
            for k, (x, y) in case.facts.get("alone_on_row", {}).items():
                X, Y = Z.centres(case.transform, *case.raster.shape)
                assert [(r, c) for r, c in pix[k] if Y[r, c] == y] == [(r, c) for r, c in pix[k] if Y[r, c] == y and X[r, c] == x] != []
            for k in case.facts.get("refused", []):
                assert want.status[k] == 2
            for k in case.facts.get("over", []):
                assert case.rings[k].shape[0] > Z.RING_CAP and want.status[k] == 0
            if "nan_crowns" in case.facts:
                assert np.isnan(want.stats[case.facts["nan_crowns"]]).all() and not np.isnan(want.stats[case.facts["clean_crowns"]]).any()
                assert all(h > 0 for h in case.facts["hits"])
                first_nan = [next((r, c) for r, c in pix[k] if np.isnan(case.raster[r, c])) for k in case.facts["nan_crowns"]]
                assert [tuple(p) for p in want.pos[case.facts["nan_crowns"]]] == first_nan
            for k, p in case.facts.get("first_max", {}).items():
                assert tuple(want.pos[k]) == p and want.stats[k, 1] == 9.0 and sum(case.raster[r, c] == 9.0 for r, c in pix[k]) >= 2
            if "first_zero_negative" in case.facts:
                col = want.stats[:, case.facts["which"]]
                assert (col == 0).all() and np.signbit(col).tolist() == case.facts["first_zero_negative"]
                for k in range(len(case.rings)):                      # and a zero of the other sign does lie inside, later
                    assert any(case.raster[r, c] == 0 and np.signbit(case.raster[r, c]) != np.signbit(col[k]) for r, c in pix[k])
            if case.repeat is not None:
                assert case.repeat.size > Z.IN_FLIGHT and np.unique(case.repeat).size == len(case.rings) == 300


def test_near_boundary_cases_are_what_they_were_designed_to_be():
    """For every near-boundary configuration the rational orientation of the centre against the edge is exactly zero, or not zero,
    as the case says; "tiny" ones are not zero yet below the float filter's error bound (1e-15 of the two products), so the
    double-double path decides them."""
    seen = set()
    for family in Z.FAMILIES:
        for i, case in enumerate(Z.cases(family)):
            X, Y = Z.centres(case.transform, *case.raster.shape)
            for k, edge, (r, c), kind in case.facts.get("near", []):
                ring = case.rings[k]
                a, b = ring[edge], ring[(edge + 1) % ring.shape[0]]
                det = Z.orientation_exact(a[0], a[1], b[0], b[1], X[r, c], Y[r, c])
                products = abs((Fraction(a[0]) - Fraction(X[r, c])) * (Fraction(b[1]) - Fraction(Y[r, c]))) + \
                    abs((Fraction(a[1]) - Fraction(Y[r, c])) * (Fraction(b[0]) - Fraction(X[r, c])))
                print(f"{case.name} ring {k} edge {edge} pixel ({r}, {c}): {kind}, determinant {float(det):.3e}, products {float(products):.3e}")
                if kind == "zero":
                    assert det == 0 and (r, c) in Z.inside(family, i)[k]
                elif kind == "tiny":
                    assert det != 0 and abs(det) < Fraction(1, 10 ** 15) * products / 2
                else:
                    assert det != 0 and abs(det) < Fraction(1, 10 ** 6)
                seen.add(kind)
    assert seen == {"zero", "nonzero", "tiny"}


def _direct(raster, transform, xy, start, n=None, n_xy=None, rows=None, cols=None, null=None, xy_ptr=None):
    """One td_crown_zonal call on host arrays, outputs pre-filled with sentinels → (status code, out, pos, status)."""
    lib = _lib.load()
    k = start.size - 1
    out, pos, status = np.full((k, 4), -7.0, np.float32), np.full((k, 3), -7, np.int32), np.full(k, -7, np.int32)
    tr = (C.c_double * 6)(*transform)
    ptr = {"raster": raster.ctypes.data, "xy": xy.ctypes.data if xy_ptr is None else xy_ptr, "start": start.ctypes.data, "out": out.ctypes.data,
           "pos": pos.ctypes.data, "status": status.ctypes.data}
    if null:
        ptr[null] = None
    st = lib.td_crown_zonal(ptr["raster"], raster.shape[0] if rows is None else rows, raster.shape[1] if cols is None else cols, tr, ptr["xy"],
                            xy.shape[0] if n_xy is None else n_xy, ptr["start"], k if n is None else n, ptr["out"], ptr["pos"], ptr["status"])
    return st, out, pos, status


def test_starts_outside_xy_are_refused_per_crown_and_bad_calls_before_anything_runs():
    case = Z.cases("boundary")[0]
    raster = np.array(case.raster)
    xy = np.ascontiguousarray(np.concatenate(case.rings[:3]))
    m = [r.shape[0] for r in case.rings[:3]]
    good = np.array([0, m[0], m[0] + m[1], m[0] + m[1] + m[2]], np.int64)
    want = Z.expected("boundary", 0)
    st, out, pos, status = _direct(raster, case.transform, xy, good)
    assert st == 0 and status.tolist() == [0, 0, 0] and pos[:, 0].tolist() == want.count[:3].tolist()
    # a start below zero, an end past xy, a decreasing pair: that crown is refused, its neighbours are computed
    for start, refused in ((np.array([-1, m[0], m[0] + m[1], good[3]], np.int64), [0]), (np.array([0, m[0], m[0] + m[1], good[3] + 1], np.int64), [2]),
                           (np.array([0, m[0] + m[1], m[0], good[3]], np.int64), [1])):
        st, o, p, s = _direct(raster, case.transform, xy, start)
        assert st == 0
        for k in range(3):
            if k in refused:
                assert s[k] == 2 and np.isnan(o[k]).all() and (p[k] == -1).all()
            elif start[k] == good[k] and start[k + 1] == good[k + 1]:
                assert s[k] == 0 and np.array_equal(o[k], out[k]) and (p[k] == pos[k]).all()
    for kwargs in ({"null": "raster"}, {"null": "xy"}, {"null": "start"}, {"null": "out"}, {"null": "pos"}, {"null": "status"}, {"n": -1}, {"rows": 0},
                   {"cols": 0}, {"cols": -3}, {"n_xy": -1}, {"xy_ptr": xy.ctypes.data + 4}):
        st, o, p, s = _direct(raster, case.transform, xy, good, **kwargs)
        assert st == _lib.ERR_INVALID and b"td_crown_zonal" in _lib.load().td_last_error(), kwargs
        assert (o == -7).all() and (p == -7).all() and (s == -7).all(), kwargs
    st, o, p, s = _direct(raster, case.transform, xy, good, n=0)
    assert st == 0 and (o == -7).all() and (p == -7).all() and (s == -7).all()


def test_wrapper_shapes_and_closed_rings():
    case = Z.cases("concave")[0]
    closed = [np.concatenate([r, r[:1]]) for r in case.rings]
    a, b = _host(case), P.crown_zonal_stats(np.array(case.raster), case.transform, closed, device=None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert [x.shape for x in a] == [(2, 4), (2,), (2, 2), (2,)] and [x.dtype for x in a] == [np.float32, np.int32, np.int32, np.int32]
    e = P.crown_zonal_stats(np.array(case.raster), case.transform, [], device=None)
    assert [x.shape for x in e] == [(0, 4), (0,), (0, 2), (0,)]


def test_crown_statistics_setting():
    assert P.crown_statistics_setting() == "circle" and P.crown_statistics_setting(None) == "circle"
    assert P.crown_statistics_setting("circle") == "circle" and P.crown_statistics_setting("polygon") == "polygon"
    for bad in ("Polygon", "polygons", "", "true", True, False, 1, 0, ["polygon"]):
        with pytest.raises(ValueError, match="crown_statistics must be 'circle' or 'polygon'"):
            P.crown_statistics_setting(bad)


def test_resume_parameters_gain_the_key_only_for_polygon(tmp_path):
    base = {"tile_width": 50, "tile_height": 50, "buffer": 20, "confidence_threshold": 0.3, "containment_threshold": 0.9, "height_threshold": 3,
            "iou_threshold": 0.5, "confidence_threshold_stitching": 0.3, "area_threshold": 1}
    absent, _ = P.load_recovery_data_with_params(str(tmp_path), dict(base))
    circle, _ = P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_statistics="circle"))
    polygon, _ = P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_statistics="polygon"))
    assert absent == circle and "crown_statistics" not in absent and list(absent) == list(P._PARAM_KEYS)
    assert polygon == dict(absent, crown_statistics="polygon")
    with pytest.raises(ValueError, match="crown_statistics"):
        P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_statistics="ring"))
    # a resume file written without the key still resumes a circle run, and does not resume a polygon run
    P.save_recovery_data_with_params(str(tmp_path), absent, {"a.gpkg"})
    assert P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_statistics="circle"))[1] == {"a.gpkg"}
    assert P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_statistics="polygon"))[1] == set()
