"""The exact oracle for the intersection area of two simple polygon rings, and the seeded cases the ring-IoU tests share.

A deliberately different algorithm from the code under test (csrc/ring_clip.h: fan triangles, clipped pairwise, float64): the
SLAB decomposition in ``fractions.Fraction``. Cut the plane at every vertex y and at the y of every crossing of an edge of P with
an edge of Q. Inside a slab no two edges cross, so both polygons are sets of x-intervals whose ends are linear in y, and so is the
total width of the overlap of the two sets: a slab contributes (overlap width at mid-height) x height, exactly. Floats convert to
rationals without loss: the result is the true area of the intersection of the polygons as given.

``scale(P, Q)`` = sum_i sum_j min(|tri_i|, |tri_j|) over the fan triangles about the prescribed origin O (the centre of the
intersection of the two bounding boxes), in float64: an upper bound of the sum of the magnitudes of the terms the code under test
adds (a triangle intersection is no larger than either triangle) that does not come from that code.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np


def _frac(ring):
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in np.asarray(ring, dtype=np.float64).reshape(-1, 2)]


def _edges(pts):
    return [(pts[k], pts[(k + 1) % len(pts)]) for k in range(len(pts))]


def _crossing_y(e, f):
    """y of the single point where segments e and f meet when they are not parallel, else None."""
    (ax, ay), (bx, by) = e
    (cx, cy), (dx, dy) = f
    rx, ry, sx, sy = bx - ax, by - ay, dx - cx, dy - cy
    den = rx * sy - ry * sx
    if den == 0:
        return None
    t = ((cx - ax) * sy - (cy - ay) * sx) / den
    u = ((cx - ax) * ry - (cy - ay) * rx) / den
    if 0 <= t <= 1 and 0 <= u <= 1:
        return ay + t * ry
    return None


def _intervals(edges, y0, y1, ym):
    """The x-intervals of a polygon at height ym inside the slab (y0, y1): edges that span the slab, paired up in x order."""
    xs = []
    for (ax, ay), (bx, by) in edges:
        if ay == by:
            continue
        lo, hi = (ay, by) if ay < by else (by, ay)
        if lo <= y0 and hi >= y1:
            xs.append(ax + (bx - ax) * (ym - ay) / (by - ay))
    xs.sort()
    assert len(xs) % 2 == 0, "a simple ring crosses a horizontal line an even number of times"
    return [(xs[k], xs[k + 1]) for k in range(0, len(xs), 2)]


def exact_area(ring):
    p = _frac(ring)
    return abs(sum(a[0] * b[1] - a[1] * b[0] for a, b in _edges(p))) / 2


def exact_intersection_area(P, Q):
    """Area of the intersection of the open rings P and Q (simple, either winding) as a Fraction."""
    ep, eq = _edges(_frac(P)), _edges(_frac(Q))
    ys = {a[1] for a, _ in ep} | {a[1] for a, _ in eq}
    for e in ep:
        for f in eq:
            y = _crossing_y(e, f)
            if y is not None:
                ys.add(y)
    ys = sorted(ys)
    total = Fraction(0)
    for y0, y1 in zip(ys[:-1], ys[1:]):
        ym = (y0 + y1) / 2
        ip, iq = _intervals(ep, y0, y1, ym), _intervals(eq, y0, y1, ym)
        width = Fraction(0)
        for a, b in ip:
            for c, d in iq:
                lo, hi = max(a, c), min(b, d)
                if hi > lo:
                    width += hi - lo
        total += width * (y1 - y0)
    return total


def exact_iou(P, Q):
    inter = exact_intersection_area(P, Q)
    union = exact_area(P) + exact_area(Q) - inter
    return inter / union


def is_simple(ring):
    """No two non-adjacent edges of the open ring meet and adjacent ones meet only in their shared vertex (exact). Edges of zero
    length are refused."""
    p = _frac(ring)
    e = _edges(p)
    n = len(e)
    if n < 3 or any(a == b for a, b in e):
        return False

    def orient(a, b, c):
        v = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        return (v > 0) - (v < 0)

    def on(a, b, c):        # c on the closed segment ab, given collinear
        return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])

    def meet(a, b, c, d):
        o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
        if o1 != o2 and o3 != o4:
            return True
        return (o1 == 0 and on(a, b, c)) or (o2 == 0 and on(a, b, d)) or (o3 == 0 and on(c, d, a)) or (o4 == 0 and on(c, d, b))

    for i in range(n):
        for j in range(i + 1, n):
            (a, b), (c, d) = e[i], e[j]
            if j == i + 1 or (i == 0 and j == n - 1):
                s, x, y = (b, a, d) if j == i + 1 else (a, b, c)      # shared vertex s, the two far ends
                if orient(s, x, y) == 0 and (x[0] - s[0]) * (y[0] - s[0]) + (x[1] - s[1]) * (y[1] - s[1]) > 0:
                    return False                                       # a spike: the two edges fold back onto each other
                continue
            if meet(a, b, c, d):
                return False
    return True


def origin(P, Q):
    """(the prescribed origin: the centre of the intersection of the two float64 bounding boxes; whether that intersection has
    positive width and height)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    x0, x1 = max(P[:, 0].min(), Q[:, 0].min()), min(P[:, 0].max(), Q[:, 0].max())
    y0, y1 = max(P[:, 1].min(), Q[:, 1].min()), min(P[:, 1].max(), Q[:, 1].max())
    return np.array([(x0 + x1) / 2, (y0 + y1) / 2]), bool(x1 > x0 and y1 > y0)


def shoelace_magnitude(R, o):
    """1/2 sum_k (|x_k y_k+1| + |y_k x_k+1|) on v - o: what the rounding error of a float64 shoelace sum is relative to."""
    v = np.asarray(R, dtype=np.float64) - o
    w = np.roll(v, -1, axis=0)
    return 0.5 * float((np.abs(v[:, 0] * w[:, 1]) + np.abs(v[:, 1] * w[:, 0])).sum())


def scale(P, Q):
    """sum_i sum_j min(|tri_i|, |tri_j|) about the prescribed origin, float64 (0 when the boxes do not overlap)."""
    o, overlap = origin(P, Q)
    if not overlap:
        return 0.0
    def fan(R):
        v = np.asarray(R, dtype=np.float64) - o
        w = np.roll(v, -1, axis=0)
        return 0.5 * np.abs(v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
    return float(np.minimum(fan(P)[:, None], fan(Q)[None, :]).sum())


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def star(rng, n, centre, r_lo, r_hi, convex=False):
    """A ring that is star-shaped about ``centre``: n vertices at increasing angles (jittered inside their sector), radii in
    [r_lo, r_hi]; ``convex``: on one ellipse instead."""
    ang = (np.arange(n) + rng.uniform(0.15, 0.85, n)) * (2 * np.pi / n) + rng.uniform(0, 2 * np.pi)
    if convex:
        a, b = rng.uniform(r_lo, r_hi, 2)
        return np.stack([centre[0] + a * np.cos(ang), centre[1] + b * np.sin(ang)], axis=1)
    r = rng.uniform(r_lo, r_hi, n)
    return np.stack([centre[0] + r * np.cos(ang), centre[1] + r * np.sin(ang)], axis=1)


def _square(x, y, s):
    return np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s]], dtype=np.float64)


@lru_cache(maxsize=None)
def cases():
    """((name, P, Q), ...): open rings as float64 [m, 2], every one simple (tests/test_ring_iou.py checks it exactly). Seeded."""
    rng = np.random.default_rng(20240611)
    out = []
    for k in range(3):
        out.append((f"convex{k}", star(rng, int(rng.integers(3, 25)), (0, 0), 2, 6, True), star(rng, int(rng.integers(3, 25)), rng.uniform(-2, 2, 2), 2, 6, True)))
    for k in range(4):
        out.append((f"star{k}", star(rng, int(rng.integers(5, 25)), (0, 0), 2, 7), star(rng, int(rng.integers(5, 25)), rng.uniform(-3, 3, 2), 2, 7)))
    for k in range(2):
        c = rng.uniform(-0.3, 0.3, 2)
        out.append((f"nested{k}", star(rng, int(rng.integers(5, 25)), (0, 0), 5, 8), star(rng, int(rng.integers(3, 25)), c, 1, 3)))
    # the boxes overlap ([1, 10] squared), the outlines are disjoint: x + y <= 10 against x + y >= 11.5
    out.append(("boxes_only0", np.array([[0, 0], [10, 0], [0, 10.0]]), np.array([[10.5, 10.5], [1, 10.5], [10.5, 1.0]])))
    out.append(("boxes_only1", np.array([[0, 0], [10, 0], [10, 1], [1, 1], [1, 10], [0, 10.0]]), _square(2.5, 2.5, 6) + rng.uniform(0, 0.5, 2)))
    out.append(("shared_edge0", _square(0, 0, 1), _square(1, 0, 1)))
    out.append(("shared_edge1", np.array([[0, 0], [4, 1], [3, 5.0]]), np.array([[4, 1], [7, 6], [3, 5.0]])))
    out.append(("shared_edge_inside", _square(0, 0, 4), np.array([[0, 1], [2, 1], [2, 3], [0, 3.0]])))       # Q inside P along P's left edge
    out.append(("shared_vertex0", _square(0, 0, 1), _square(1, 1, 1)))
    out.append(("shared_vertex1", np.array([[0, 0], [3, 0.5], [1, 2.0]]), np.array([[3, 0.5], [5, 3], [2.5, 3.0]])))
    s = star(rng, 17, (1.5, -2.5), 2, 7)
    out.append(("identical", s, s.copy()))
    out.append(("identical_rotated", s, np.roll(s, 5, axis=0)))
    out.append(("identical_reversed", s, np.roll(s[::-1], 3, axis=0)))
    for k in range(3):
        snap = lambda r: np.round(r * 4) / 4
        out.append((f"grid{k}", snap(star(rng, int(rng.integers(4, 13)), (0, 0), 3, 7)), snap(star(rng, int(rng.integers(4, 13)), rng.integers(-8, 9, 2) / 4, 3, 7))))
    out.append(("grid_squares_nested", _square(0, 0, 4), _square(1, 1, 2)))
    out.append(("grid_squares_offset", _square(0, 0, 4), _square(2, 0, 4)))
    for k in range(2):
        out.append((f"winding{k}", star(rng, int(rng.integers(5, 25)), (0, 0), 2, 7)[::-1].copy(), star(rng, int(rng.integers(5, 25)), rng.uniform(-3, 3, 2), 2, 7)))
    out.append(("winding_both", star(rng, 9, (0, 0), 2, 7)[::-1].copy(), star(rng, 11, (1, 1), 2, 7)[::-1].copy()))
    utm = np.array([4e5, 5e6])
    for k in range(3):
        out.append((f"utm{k}", star(rng, int(rng.integers(5, 25)), utm + rng.uniform(0, 500, 2), 2, 7), None))
        c = out[-1][1].mean(axis=0)
        out[-1] = (out[-1][0], out[-1][1], star(rng, int(rng.integers(5, 25)), c + rng.uniform(-3, 3, 2), 2, 7))
    out.append(("utm_grid", np.round((star(rng, 10, (0, 0), 3, 7)) * 4) / 4 + utm, np.round(star(rng, 8, (1, 0.5), 3, 7) * 4) / 4 + utm))
    out.append(("sliver0", np.array([[0, 0], [100, 0.01], [100, 0.02]]), np.array([[50, -5], [50.01, -5], [50.005, 5.0]])))
    out.append(("sliver1", np.array([[0, 0], [1e3, 1e-3], [0, 2e-3]]), np.array([[1, -1], [999, 1.001], [999, 1.002], [1, -0.999]])))
    out.append(("sliver_in_star", star(rng, 20, (0, 0), 4, 9), np.array([[-12, 0.001], [12, 0.0015], [12, 0.002]])))
    return tuple((name, np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)) for name, p, q in out)


@lru_cache(maxsize=None)
def exact_results():
    """name → (exact intersection area, exact area of P, exact area of Q) as Fractions; computed once per session."""
    return {name: (exact_intersection_area(p, q), exact_area(p), exact_area(q)) for name, p, q in cases()}


def regular(n, centre=(0.0, 0.0), r=3.0, phase=0.1):
    ang = phase + np.arange(n) * (2 * np.pi / n)
    return np.stack([centre[0] + r * np.cos(ang), centre[1] + r * np.sin(ang)], axis=1)


WAVE_SHAPES = ((3, 3), (7, 9), (8, 8), (5, 13), (3, 43), (3, 4), (4, 4))      # m x n: term counts around one wave of 64 lanes


@lru_cache(maxsize=None)
def wave_cases():
    """((name, P, Q), ...) with the vertex counts of WAVE_SHAPES: irregular convex rings, overlapping."""
    rng = np.random.default_rng(77)
    return tuple((f"wave{m}x{n}", star(rng, m, (0, 0), 2, 5, True), star(rng, n, rng.uniform(-1, 1, 2), 2, 5, True)) for m, n in WAVE_SHAPES)


def crown_scene(n, seed):
    """n crowns as CLOSED rings (the way Layer.rings() gives them) with scores, at UTM coordinates: star-shaped crowns of 6 - 10
    vertices on a jittered grid (neighbours overlap a little), every fourth followed by a shrunk and shifted near-duplicate
    (IoU around 0.7 - 0.95), every seventh by an exact twin with another starting vertex or direction, every eleventh a tiny ring
    (area below 1). Scores have two decimals, so ties happen. Seeded."""
    rng = np.random.default_rng(seed)
    side = max(1, int(np.ceil(np.sqrt(n))))
    rings, scores = [], []
    k = 0
    while len(rings) < n:
        c = np.array([412000.0 + 4.5 * (k % side), 5318000.0 + 4.5 * (k // side)]) + rng.uniform(-0.8, 0.8, 2)
        ring = star(rng, int(rng.integers(6, 11)), c, 0.25 if k % 11 == 10 else 2.0, 0.4 if k % 11 == 10 else 3.2)
        rings.append(ring)
        if k % 4 == 1:
            rings.append(c + (ring - c) * rng.uniform(0.86, 0.98) + rng.uniform(-0.08, 0.08, 2))
        if k % 7 == 3:
            twin = np.roll(ring, int(rng.integers(1, 5)), axis=0)
            rings.append(twin[::-1].copy() if k % 2 else twin)
        k += 1
    rings = rings[:n]
    scores = [float(v) for v in np.round(rng.uniform(0.05, 1.0, n), 2)]
    return [np.concatenate([r, r[:1]]) for r in rings], scores
