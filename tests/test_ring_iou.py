"""td_ring_pairs_area (the host twin of the ring-pair kernel, csrc/ring_clip.h) against the exact slab oracle of
tests/ring_iou_ref.py, on the CPU.

The bound: |inter - exact| <= K * 2^-52 * scale(P, Q), scale = sum_i sum_j min(|tri_i|, |tri_j|) about the prescribed origin.
Measured on the committed cases (ring_iou_ref.cases() and wave_cases(), host library, x86-64): the largest ratio
|inter - exact| / (2^-52 * scale) is 30.75, on ``sliver_in_star`` — a sliver's fan triangles are tiny, so scale is tiny, while the
clip's rounding is relative to the coordinates (12) — and 0.63 on every other case. K = ceil(4 x 30.75) = 123: four times the
measured maximum, because the cases are a finite sample of rounding patterns and the error grows like a random walk in the term
count. The ring areas are held to 16 * 2^-52 * (1/2 sum |x_k y_k+1| + |y_k x_k+1| on v - O): two roundings of v - O per factor,
one per product, one per difference and at most seven additions (one in the lane, six in the butterfly) for rings of up to 64
vertices make 11 half-units; 16 leaves the rest to the final halving and the oracle's own conversion (none: both are exact).
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_iou_ref as R  # noqa: E402
from treedetection_amd import _lib  # noqa: E402
from treedetection_amd import cleaning as CL  # noqa: E402

K = 123
ULP = Fraction(1, 2 ** 52)
ALL = {name: (p, q) for name, p, q in R.cases() + R.wave_cases()}


def host(p, q):
    xa, sa = CL.pack_rings([p])
    xb, sb = CL.pack_rings([q])
    out, status = CL.ring_pairs_area_packed(xa, sa, xb, sb, [[0, 0]], None)
    assert status[0] == 0
    return out[0]


@pytest.fixture(scope="module")
def exact():
    return {name: (R.exact_intersection_area(p, q), R.exact_area(p), R.exact_area(q)) for name, (p, q) in ALL.items()}


def test_the_oracle_knows_areas_that_can_be_worked_out_by_hand():
    sq = lambda x, y, s: np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s]], dtype=np.float64)
    assert R.exact_intersection_area(sq(0, 0, 4), sq(2, 0, 4)) == 8
    assert R.exact_intersection_area(sq(0, 0, 4), sq(1, 1, 2)) == 4
    assert R.exact_intersection_area(sq(0, 0, 1), sq(1, 0, 1)) == 0 and R.exact_intersection_area(sq(0, 0, 1), sq(5, 5, 1)) == 0
    tri = np.array([[0, 0], [4, 0], [0, 4.0]])
    assert R.exact_intersection_area(tri, sq(0, 0, 2)) == 4 and R.exact_intersection_area(tri, sq(1, 1, 2)[::-1]) == 2 and R.exact_intersection_area(tri, sq(1, 1, 1)) == 1
    # a non-convex ring: the U's notch holds none of the bar that crosses it except where the two arms are
    u = np.array([[0, 0], [6, 0], [6, 4], [4, 4], [4, 1], [2, 1], [2, 4], [0, 4.0]])
    bar = np.array([[-1, 2], [7, 2], [7, 3], [-1, 3.0]])
    assert R.exact_area(u) == 18 and R.exact_intersection_area(u, bar) == 4
    assert R.exact_iou(sq(0, 0, 4), sq(2, 0, 4)) == Fraction(8, 24)


def test_every_committed_ring_is_simple():
    for name, (p, q) in ALL.items():
        assert R.is_simple(p) and R.is_simple(q), name
    assert not R.is_simple(np.array([[0, 0], [2, 2], [2, 0], [0, 2.0]]))        # a bow-tie


@pytest.mark.parametrize("name", list(ALL))
def test_host_area_is_within_the_bound_of_the_exact_area(name, exact):
    p, q = ALL[name]
    inter, area_p, area_q = (float(v) for v in host(p, q))
    want, want_p, want_q = exact[name]
    bound = K * ULP * Fraction(R.scale(p, q))
    err = abs(Fraction(inter) - want)
    print(f"{name}: inter {inter!r} exact {float(want)!r} error {float(err):.3e} bound {float(bound):.3e}")
    assert err <= bound
    assert 0.0 <= inter <= min(area_p, area_q) and not np.signbit(inter)
    o, _ = R.origin(p, q)
    assert abs(Fraction(area_p) - want_p) <= 16 * ULP * Fraction(R.shoelace_magnitude(p, o))
    assert abs(Fraction(area_q) - want_q) <= 16 * ULP * Fraction(R.shoelace_magnitude(q, o))


def test_exact_expectations(exact):
    # boxes that do not overlap with positive area: +0.0, whatever the outlines do
    sq = lambda x, y, s: np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s]], dtype=np.float64)
    for p, q in ((sq(0, 0, 1), sq(5, 5, 1)), (sq(0, 0, 1), sq(1, 0, 1)), (sq(0, 0, 1), sq(1, 1, 1)), (sq(4e5, 5e6, 3), sq(4e5 - 3, 5e6, 3)[::-1])):
        out = host(p, q)
        assert out[0] == 0.0 and not np.signbit(out[0]) and out[1] == out[2] == abs(float(R.exact_area(p)))
    # outlines disjoint, boxes overlapping, and outlines that share an edge or a vertex only: exactly 0 here (every term cancels)
    for name in ("boxes_only0", "boxes_only1", "shared_edge0", "shared_edge1", "shared_vertex0", "shared_vertex1"):
        assert exact[name][0] == 0 and host(*ALL[name])[0] == 0.0, name
    # nested: the oracle says the inner area, and the host function says it within the bound
    for name in ("nested0", "nested1", "grid_squares_nested"):
        p, q = ALL[name]
        assert exact[name][0] == exact[name][2]
        assert abs(Fraction(float(host(p, q)[0])) - exact[name][2]) <= K * ULP * Fraction(R.scale(p, q))
    # identical rings, whatever the starting vertex and direction: the same three numbers, inter = the area after the clamp
    a, b, c = (host(*ALL[n]) for n in ("identical", "identical_rotated", "identical_reversed"))
    assert a[0] <= a[1] and abs(a[0] - a[1]) <= float(K * ULP) * R.scale(*ALL["identical"])
    assert np.allclose(a, b, rtol=1e-14, atol=0) and np.allclose(a, c, rtol=1e-14, atol=0)
    # squares on a grid come out exactly
    assert host(*ALL["grid_squares_offset"]).tolist() == [8.0, 16.0, 16.0] and host(*ALL["grid_squares_nested"]).tolist() == [4.0, 16.0, 4.0]


def test_argument_order_windings_and_closed_rings():
    p, q = ALL["star1"]
    a = host(p, q)
    b = host(q, p)
    bound = float(K * ULP) * R.scale(p, q)
    assert abs(a[0] - b[0]) <= 2 * bound and (a[1], a[2]) == (b[2], b[1])
    assert abs(host(p[::-1].copy(), q)[0] - a[0]) <= 2 * bound
    closed = [np.concatenate([r, r[:1]]) for r in (p, q)]
    iou, areas = CL.ring_pairs_iou(closed[:1], closed[1:], [[0, 0]], None)          # closed rings lose their repeated vertex
    assert areas[0].tolist() == a.tolist() and iou[0] == a[0] / ((a[1] + a[2]) - a[0])
    one, areas = CL.ring_pairs_iou(closed, closed, [[0, 0], [1, 1], [0, 1]], None)  # one list on both sides, self pairs
    assert abs(one[0] - 1) <= 1e-14 and abs(one[1] - 1) <= 1e-14 and one[2] == iou[0]


def test_many_pairs_two_ring_sets_and_refused_pairs():
    names = list(ALL)[:12]
    ring_a = [ALL[n][0] for n in names]
    ring_b = [ALL[n][1] for n in names] + [np.array([[0, 0], [1, 1.0]])]         # the last ring of B has two vertices
    xa, sa = CL.pack_rings(ring_a)
    xb, sb = CL.pack_rings(ring_b)
    pairs = [[k, k] for k in range(12)] + [[3, 3], [12, 0], [0, 13], [-1, 0], [0, 12]]
    out, status = CL.ring_pairs_area_packed(xa, sa, xb, sb, pairs, None)
    assert status.tolist() == [0] * 13 + [2, 2, 2, 2]
    for k, n in enumerate(names):
        assert out[k].tolist() == host(*ALL[n]).tolist()
    assert out[12].tolist() == out[3].tolist() and np.isnan(out[13:]).all()
    with pytest.raises(ValueError, match="refused"):
        CL.ring_pairs_iou(ring_a, ring_b, [[0, 12]], None)
    bad = ring_a[0].copy()
    bad[1, 0] = np.nan
    out, status = CL.ring_pairs_area_packed(*CL.pack_rings([bad, ring_a[1]]), *CL.pack_rings(ring_b), [[0, 0], [1, 0]], None)
    assert status.tolist() == [2, 0] and np.isnan(out[0]).all() and not np.isnan(out[1]).any()
    bad[1, 0] = np.inf
    assert CL.ring_pairs_area_packed(*CL.pack_rings([bad]), *CL.pack_rings(ring_b), [[0, 0]], None)[1].tolist() == [2]
    out, status = CL.ring_pairs_area_packed(xa, sa, xb, sb, np.zeros((0, 2), np.int32), None)
    assert out.shape == (0, 3) and status.shape == (0,)


def test_entry_point_validation():
    lib = _lib.load()
    buf = np.zeros(16)
    start = np.array([0, 4], np.int64)
    pairs = np.zeros((1, 2), np.int32)
    out, status = np.zeros(3), np.zeros(1, np.int32)
    args = [buf.ctypes.data, start.ctypes.data, 1, buf.ctypes.data, start.ctypes.data, 1, pairs.ctypes.data, 1, out.ctypes.data, status.ctypes.data]
    for k in (0, 1, 3, 4, 6, 8, 9):
        a = list(args)
        a[k] = None
        assert lib.td_ring_pairs_area(*a) == _lib.ERR_INVALID and b"null" in lib.td_last_error()
    a = list(args)
    a[7] = -1
    assert lib.td_ring_pairs_area(*a) == _lib.ERR_INVALID and b"n_pairs" in lib.td_last_error()
    a[7] = 0
    out[:] = 7
    assert lib.td_ring_pairs_area(*a) == 0 and out.tolist() == [7, 7, 7]
    with pytest.raises(ValueError, match="start_a"):
        CL.ring_pairs_area_packed(np.zeros((4, 2)), [0, 5], np.zeros((4, 2)), [0, 4], [[0, 0]], None)


def test_candidate_pairs_host_equals_brute_force():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 60):
        lo = rng.uniform(0, 30, (n, 2))
        b = np.concatenate([lo, lo + rng.uniform(0.5, 8, (n, 2))], axis=1)
        if n == 60:
            b[7] = b[3]                                             # identical boxes
            b[9, :2] = b[8, 2:]                                     # touching in a corner only: no positive area
            b[11] = [b[10, 2], b[10, 1], b[10, 2] + 1, b[10, 3]]    # touching along an edge only
        want = [(i, j) for i in range(n) for j in range(i + 1, n)
                if min(b[i, 2], b[j, 2]) > max(b[i, 0], b[j, 0]) and min(b[i, 3], b[j, 3]) > max(b[i, 1], b[j, 1])]
        got = CL.candidate_pairs_host(b)
        assert got.dtype == np.int32 and got.shape == (len(want), 2) and [tuple(p) for p in got.tolist()] == want
