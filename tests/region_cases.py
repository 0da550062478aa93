"""Crafted configurations for the outline predicates (data only, no tests): every family is one region (polygons with holes) and a
list of closed query rings. tests/test_region_cases.py proves each family against the exact rational oracle (oracle/region_ref.py)
and the host td_region_relate; tests/test_region_relate_gpu.py then holds td_region_relate_dev to the host's flags on the same
families, so the device test stands on cases known to be right.

A family: {"name", "forest", "queries", "want": [(intersects, within)] or None (the oracle says), "beyond": indices of the queries
built beyond a fixed capacity of the kernel (the only ones it may leave to the host), "mixed": True when all three outcomes must
occur among the queries}.
"""
import numpy as np

from treedetection_amd import _lib

UTM = np.array([500000.0, 5600000.0])       # x ~ 5e5, y ~ 5.6e6: one ulp is 2^-34 in x and 2^-30 in y
LATTICE_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
QCAP, MCAP, RCAP = _lib.RELATE_QUERY_CAP, _lib.RELATE_MEET_CAP, _lib.RELATE_RING_CAP


def sq(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]], float)


def family(name, forest, queries, want=None, beyond=(), mixed=False):
    return {"name": name, "forest": forest, "queries": queries, "want": want, "beyond": sorted(beyond), "mixed": mixed}


def moved(forest, queries, offset, snap=None):
    """Everything translated by ``offset``; with ``snap`` the coordinates first go to the 1/snap lattice, so collinear stays collinear."""
    f = (lambda r: np.round(np.asarray(r, float) * snap) / snap + offset) if snap else (lambda r: np.asarray(r, float) + offset)
    return [[f(r) for r in poly] for poly in forest], [f(q) for q in queries]


# ---- the known answers of tests/test_region.py, restated ------------------------------------------------------------------------
FOREST = [
    [sq(0, 0, 10, 10), sq(4, 4, 6, 6)],          # A: square with a hole
    [sq(10, 0, 20, 10)],                         # B: shares the edge x = 10 with A
    [sq(30, 0, 40, 10)],                         # C: apart
    [sq(4.5, 4.5, 5.5, 5.5)],                    # D: an island inside A's hole
]
KNOWN = [
    ("inside A", sq(1, 1, 2, 2), True, True),
    ("outside everything", sq(22, 1, 28, 2), False, False),
    ("across the shared edge of A and B", sq(8, 1, 12, 2), True, True),
    ("across A's outer edge", sq(-1, 1, 1, 2), True, False),
    ("touching A from outside along an edge", sq(-2, 1, 0, 2), True, False),
    ("touching A from outside at a corner", sq(-2, -2, 0, 0), True, False),
    ("inside the hole, clear of the island", sq(4.1, 4.1, 4.4, 4.4), False, False),
    ("inside the hole, touching its rim", sq(4, 4.1, 4.3, 4.4), True, False),
    ("inside the island", sq(4.8, 4.8, 5.2, 5.2), True, True),
    ("covering the whole hole", sq(3, 3, 7, 7), True, False),
    ("covering island and part of the hole", sq(4.3, 4.3, 5.7, 5.7), True, False),
    ("A and B together, exactly", sq(0, 0, 20, 10), True, False),
    ("inside B up to its boundary", sq(10, 0, 20, 10), True, True),
    ("spanning the gap between B and C", sq(15, 1, 35, 2), True, False),
    ("containing C entirely", sq(29, -1, 41, 11), True, False),
    ("a sliver along the shared edge", sq(9.9, 2, 10.1, 8), True, True),
    ("vertex on A's boundary, rest inside", np.array([[0, 5], [2, 4], [2, 6], [0, 5]], float), True, True),
]
assert len(KNOWN) == 17


def _blob(rng, cx, cy, r, n):
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = r * rng.uniform(0.6, 1.0, n)
    ring = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    return np.concatenate([ring, ring[:1]])


def lattice(seed):
    """Star-shaped patches (some with holes, overlapping each other) and small query rings on a 0.25 lattice: vertices on edges,
    shared vertices and collinear overlaps occur (tests/test_region.py: test_matches_oracle_on_random_configurations)."""
    rng = np.random.default_rng(seed)
    forest = []
    for _ in range(8):
        cx, cy = rng.uniform(0, 40, 2)
        shell = np.round(_blob(rng, cx, cy, rng.uniform(4, 10), int(rng.integers(5, 12))) * 4) / 4
        poly = [shell]
        if rng.random() < 0.5:
            poly.append(np.round(_blob(rng, cx, cy, 1.5, 5) * 4) / 4)
        forest.append(poly)
    queries = []
    for _ in range(70):
        cx, cy = rng.uniform(-2, 42, 2)
        q = np.round(_blob(rng, cx, cy, rng.uniform(0.5, 3), int(rng.integers(3, 8))) * 4) / 4
        if abs(np.dot(q[:-1, 0], q[1:, 1]) - np.dot(q[1:, 0], q[:-1, 1])) > 0:
            queries.append(q)
    return forest, queries


# ---- one ulp off an edge: the filter of the orientation test cannot decide, the double-double branch does ------------------------
def ulp_family(name, offset):
    o = np.asarray(offset, float)
    tri = [np.array([[0, 0], [7, -5], [7, 3], [0, 0]], float) + o]          # the edge (7, 3) -> (0, 0) carries (3.5, 1.5)
    on = np.array([3.5, 1.5]) + o
    up = np.array([on[0], np.nextafter(on[1], np.inf)])                      # one ulp outside
    dn = np.array([on[0], np.nextafter(on[1], -np.inf)])                     # one ulp inside
    lf = np.array([np.nextafter(on[0], -np.inf), on[1]])                     # one ulp outside, in x
    queries, want = [], []
    for apex, outside_touches, inside_within in ((on, True, True), (up, False, False), (dn, True, True), (lf, False, False)):
        queries.append(np.array([apex, np.array([3, 4]) + o, np.array([4, 4]) + o, apex]))       # the rest outside the triangle
        want.append((outside_touches, False))
        queries.append(np.array([apex, np.array([5, 0]) + o, np.array([5, -1]) + o, apex]))      # the rest inside it
        want.append((True, inside_within))
    return family(name, [tri], queries, want)


# ---- capacities ------------------------------------------------------------------------------------------------------------------
def circle(cx, cy, r, points):
    """A closed ring of ``points`` points (the closing one included)."""
    ang = 2 * np.pi * np.arange(points - 1) / (points - 1)
    ring = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)
    return np.concatenate([ring, ring[:1]])


def sizes_family():
    forest = [[sq(0, 0, 10, 10), sq(4, 4, 6, 6)]]
    queries, beyond = [], []
    for points in (63, 64, 65, QCAP - 1, QCAP, QCAP + 1):
        for c in ((2, 2, 0.5), (5, 5, 3), (0.25, 7, 1.5), (5, 5, 0.5)):      # within; around the hole; across the shell; in the hole
            if points > QCAP:
                beyond.append(len(queries))
            queries.append(circle(*c, points))
    return family("query sizes", forest, queries, beyond=beyond)


def comb_family():
    """Two interlocking combs whose teeth overlap by 0.25: A's teeth [2i, 2i + 1.25] stand on a base below, B's [2i + 1, 2i + 2.25]
    hang from one above, so the band 0 < y < 10 is covered and a sliver through it stays within the union while ONE of its edges
    crosses tooth sides at x = 1, 1.25, 2, 2.25, ...: k meetings for a sliver that ends just behind the k-th."""
    teeth = (MCAP + 1) // 4 + 2
    width = 2 * teeth + 2
    a = [[0, -2], [width, -2], [width, 0]]
    for i in reversed(range(teeth)):
        a += [[2 * i + 1.25, 0], [2 * i + 1.25, 10], [2 * i, 10], [2 * i, 0]]
    a += [[0, -2]]
    b = [[0, 12], [0, 10]]
    for i in range(teeth):
        b += [[2 * i + 1, 10], [2 * i + 1, 0], [2 * i + 2.25, 0], [2 * i + 2.25, 10]]
    b += [[width, 10], [width, 12], [0, 12]]
    forest = [[np.array(a, float)], [np.array(b, float)]]
    queries, beyond = [], []
    for k in (3, MCAP - 1, MCAP, MCAP + 1):
        m = (k + 1) // 2
        xe = m + 0.125 if k % 2 else m + 0.5
        if k > MCAP:
            beyond.append(len(queries))
        queries.append(sq(0.5, 5, xe, 5.5))
    return family("comb: meetings on one query edge", forest, queries, want=[(True, True)] * len(queries), beyond=beyond)


def rings_family():
    """k small squares inside one large parcel, each crossed by the two long edges of a sliver: k distinct region rings met."""
    ks = (2, RCAP - 1, RCAP, RCAP + 1)
    forest = [[sq(0, -5, 2 * max(ks) + 4, 15)]] + [[sq(2 * i + 1, 4, 2 * i + 2, 6)] for i in range(max(ks))]
    queries = [sq(0.5, 4.5, 2 * k + 0.5, 5) for k in ks]
    return family("rings met by one query", forest, queries, want=[(True, True)] * len(ks), beyond=[i for i, k in enumerate(ks) if k > RCAP])


def dense_family():
    """100 strips side by side: every y-bin of the index holds 200 upright edges of 100 polygons — more than a wave's 64, more than
    two waves' worth — so a crossing count runs over several rounds of the lanes and the polygons' parities change hands between
    them."""
    forest = [[sq(i, 0, i + 0.5, 10)] for i in range(100)]
    queries = [sq(0.1, 1, 0.4, 2), sq(0.6, 1, 0.9, 2), sq(0.25, 3, 0.75, 4), sq(50.1, 5, 50.4, 6), sq(99.1, 9, 99.4, 9.9), sq(99.6, 1, 99.9, 2),
               sq(30.5, 2, 31, 3), sq(30.25, 2, 31.25, 3), sq(-1, 4, 101, 5), sq(64.1, 0, 64.4, 10), sq(63.6, 4, 63.9, 5), sq(70, -1, 70.5, 11)]
    return family("dense bins", forest, queries, mixed=True)


def crowded_families():
    """320 unit squares on a 3-unit grid, as islands in a parcel and as the holes of one: 1 280 edges lie near a query that spans the
    grid, more than the kernel lists per query (1 024), so it walks the bins instead — few of them meet the query, so few pieces."""
    squares = [sq(3 * i, 3 * j, 3 * i + 1, 3 * j + 1) for i in range(20) for j in range(16)]
    parcel = sq(-10, -10, 80, 70)
    queries = [sq(-1, -1, 62, 50), sq(-1.5, -1.5, 59.5, 47.5), np.array([[-1, -1], [61, 47.5], [61, 48.5], [-1, -1]], float),
               sq(-20, 1.5, 70, 1.75), sq(1.25, 1.25, 1.75, 1.75), sq(0.25, 0.25, 0.75, 0.75), sq(-30, -30, 90, 80)]
    return [family("more edges near a query than its list: islands", [[parcel]] + [[r] for r in squares], queries,
                   want=[(True, True), (True, True), (True, True), (True, False), (True, True), (True, True), (True, False)]),
            family("more edges near a query than its list: holes", [[parcel] + squares], queries,
                   want=[(True, False), (True, False), (True, False), (True, False), (True, True), (False, False), (True, False)])]


_FAMILIES = None


def families():
    global _FAMILIES
    if _FAMILIES is not None:
        return _FAMILIES
    out = [family("known answers", FOREST, [c[1] for c in KNOWN], want=[(c[2], c[3]) for c in KNOWN])]
    f, q = moved(FOREST, [c[1] for c in KNOWN], UTM, snap=16)
    out.append(family("known answers at UTM", f, q, want=[(c[2], c[3]) for c in KNOWN]))
    for seed in LATTICE_SEEDS:
        f, q = lattice(seed)
        out.append(family(f"lattice {seed}", f, q, mixed=True))
        f, q = moved(f, q, UTM)
        out.append(family(f"lattice {seed} at UTM", f, q, mixed=True))
    out.append(ulp_family("one ulp off an edge", (0.0, 0.0)))
    out.append(ulp_family("one ulp off an edge at UTM", UTM))
    out.append(family("two overlapping polygons", [[sq(0, 0, 10, 10)], [sq(5, 0, 15, 10)]],
                      [sq(6, 1, 9, 2), sq(2, 1, 12, 2), sq(5, 0, 10, 10), sq(7, 3, 16, 4), sq(-1, -1, 16, 11)],
                      want=[(True, True), (True, True), (True, True), (True, False), (True, False)]))
    holed = [sq(0, 0, 20, 20), sq(8, 8, 12, 12)]
    out.append(family("hole inside a query, covered by another polygon", [holed, [sq(7, 7, 13, 13)]],
                      [sq(5, 5, 15, 15), sq(9, 9, 11, 11), sq(7.5, 7.5, 12.5, 12.5)], want=[(True, True)] * 3))
    out.append(family("hole inside a query, uncovered", [holed], [sq(5, 5, 15, 15), sq(9, 9, 11, 11), sq(7.5, 7.5, 12.5, 12.5)],
                      want=[(True, False), (False, False), (True, False)]))
    out.append(family("region ring loose inside a query", [[sq(4, 4, 6, 6)], [sq(20, 20, 21, 21)]],
                      [sq(0, 0, 10, 10), sq(3, 3, 22, 22), sq(7, 7, 9, 9)], want=[(True, False), (True, False), (False, False)]))
    out.append(family("disjoint in y", [[sq(0, 0, 10, 10)]], [sq(1, 20, 2, 21), sq(1, -21, 2, -20), sq(1, 10, 2, 11), sq(1, 10.5, 2, 11)],
                      want=[(False, False), (False, False), (True, False), (False, False)]))
    rep = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y1], [x0, y0]], float)
    out.append(family("zero-length query edge", [[sq(0, 0, 10, 10), sq(4, 4, 6, 6)]], [rep(1, 1, 2, 2), rep(9, 1, 11, 2), rep(10, 1, 11, 2),
                                                                                      rep(3, 3, 7, 7), rep(12, 1, 13, 2)],
                      want=[(True, True), (True, False), (True, False), (True, False), (False, False)]))
    out += [dense_family(), sizes_family(), comb_family(), rings_family()] + crowded_families()
    _FAMILIES = out
    return out
