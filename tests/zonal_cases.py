"""Shared inputs of the zonal-statistics tests (test_zonal_cases.py, test_crown_zonal_gpu.py): crafted rasters and crown rings for
td_crown_zonal / td_crown_zonal_dev, and an exact oracle in pure Python. Not a test.

THE ORACLE ALONE DECIDES EVERY CRAFTED PIXEL. No expected value below is written down by hand or taken from the code under test:
the pixel centres are formed in numpy float64 exactly as include/treedet.h states them — ``(a*(col+0.5) + b*(row+0.5)) + c``, every
operation rounded on its own — and membership is decided on those doubles in exact rational arithmetic (``fractions.Fraction``
orientation; the comparisons of doubles with doubles are exact as they stand) by the even-odd rule, half-open in y, the boundary
inside. The only shortcut is exact too: a centre outside the ring's bounding box is outside the ring, so only the centres inside the
box are tested. Minimum, maximum and position follow numpy's order (a NaN inside makes both NaN, at the position of the FIRST NaN in
row-major order; among numbers the first occurrence wins, so the first of equal zeros gives its sign); mean and population variance
are exact rationals rounded ONCE to float32. The few counts a case states (``facts``) are checked against the oracle by
test_zonal_cases.py, as are the near-boundary configurations: for each, that the rational orientation is exactly zero or non-zero as
the case was designed.

``cases(family)`` → a tuple of :class:`Case`; ``expected(family, i)`` → :class:`Expected` for case ``i``, computed once, read-only;
``inside(family, i)`` → per ring the (row, col) pairs inside, in row-major order. Rasters are at most 140 x 140; a case has at most
64 crowns, except lanes/grid_stride, which repeats 300 small crowns (the oracle runs on the 300) past the crowns one launch holds
in flight.

  boundary        a square whose edges run through pixel centres, a triangle with vertices ON centres and a hypotenuse through
                  centres, a trapezoid with a horizontal edge along a row of centres
  scanline        a diamond whose left and right vertices lie on a centre row; spikes that touch a centre row from below (apex on a
                  centre and between two) and a notch that touches one from above: no parity flip; two consecutive collinear
                  vertices on a centre row
  concave         a U and a three-tooth comb (rows cross 4 and 6 edges); the raster's largest value sits in the notch, inside the box
                  and the bounding circle, outside the ring
  winding         the concave rings reversed (identical rows); a bow-tie and a pentagram (even-odd: the pentagram's core is outside)
  clipping        rings off each side and each corner of the raster, wholly outside, a sliver between pixel centres (count 0), a
                  1 x 1 raster hit and missed
  large           northing 5.3e6, 0.2 m pixels: star rings; an edge exactly through a centre; an edge one unit in the last place of y
                  (9.3e-10 m) off a row of centres; an edge whose determinant against a centre is 2^-61: below the filter's bound,
                  decided by the double-double path
  transforms      e > 0, a < 0, both, anisotropic, rotated by four degrees (b, d != 0)
  values          NaNs (one, several, first, last, all, only in the notch of a U), ties (quantised plateaus, equal maxima placed
                  first / last), zeros of both signs over negative values, a constant raster
  lanes           boxes 1, 63, 64, 65 and 129 columns wide; one row tall; one column wide; the whole 140 x 140 raster (more runs of
                  64 pixels than the kernel keeps for its second pass); 300 crowns and duplicates repeated past the grid
  capacity        regular polygons of exactly the kernel's capacity and one vertex more; refused rings (0, 1, 2 vertices, NaN,
                  infinity) between good ones
"""
import functools
import math
from fractions import Fraction
from typing import Any, Dict, List, NamedTuple, Tuple

import numpy as np

RING_CAP = 512                 # TD_ZONAL_RING_CAP (include/treedet.h); test_zonal_cases.py holds it to _lib.ZONAL_RING_CAP
IN_FLIGHT = 4 * 2048           # crowns one launch holds in flight (crownzonal.hip: ZN_WPB waves x ZN_GRID_MAX workgroups)
UTM_X, UTM_Y = 412000.0, 5318060.0
UX, UY = 2.0 ** -34, 2.0 ** -30          # one unit in the last place of an x / a y there


class Case(NamedTuple):
    raster: np.ndarray                    # float32 [rows, cols]
    transform: Tuple[float, ...]
    rings: Tuple[np.ndarray, ...]         # float64 [m, 2], open
    name: str
    facts: Dict[str, Any]
    repeat: Any                           # None, or an index array: the rings the launch sees are rings[repeat]


class Expected(NamedTuple):
    status: np.ndarray                    # int32 [n]
    count: np.ndarray                     # int32 [n]
    pos: np.ndarray                       # int32 [n, 2]
    stats: np.ndarray                     # float32 [n, 4]: min, max, mean, variance


def _frozen(a):
    a.setflags(write=False)
    return a


def _case(name, raster, transform, rings, repeat=None, **facts):
    raster = _frozen(np.ascontiguousarray(raster, dtype=np.float32))
    assert raster.ndim == 2 and raster.shape[0] <= 140 and raster.shape[1] <= 140
    rings = tuple(_frozen(np.asarray(r, dtype=np.float64).reshape(-1, 2)) for r in rings)
    assert len(rings) <= 64 or repeat is not None
    return Case(raster, tuple(float(v) for v in transform), rings, name, facts, repeat)


def distinct(rows, cols, seed, lo=0.25, hi=1.0):
    """float32 [rows, cols] of one sign whose values all differ (a seeded permutation of an even grid over (lo, hi)): a pixel missed
    or taken in wrongly moves the minimum, the maximum or the mean; the spread is far above 2^-10 of the mean."""
    n = rows * cols
    p = np.random.default_rng(seed).permutation(n).astype(np.float64)
    out = (lo + (hi - lo) * (p + 0.5) / n).astype(np.float32).reshape(rows, cols)
    assert np.unique(out).size == n
    return out


def north_up(rows):
    """x = col + 0.5, y = rows - (row + 0.5): centres on the half-integers, exactly."""
    return (1.0, 0.0, 0.0, 0.0, -1.0, float(rows))


def centres(transform, rows, cols):
    """→ (X, Y) float64 [rows, cols]: the pixel centres as include/treedet.h forms them."""
    a, b, c, d, e, f = (np.float64(v) for v in transform)
    u = (np.arange(cols, dtype=np.float64) + 0.5)[None, :]
    v = (np.arange(rows, dtype=np.float64) + 0.5)[:, None]
    return (a * u + b * v) + c, (d * u + e * v) + f


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def star(rng, cx, cy, r_lo, r_hi, m):
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    rad = rng.uniform(r_lo, r_hi, m)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def orientation_exact(ax, ay, bx, by, px, py) -> Fraction:
    """(b - a) x (p - a) of six doubles, exactly."""
    ax, ay, bx, by, px, py = (Fraction(float(v)) for v in (ax, ay, bx, by, px, py))
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _edge_rule(a, b, p):
    """0 nothing, 1 p on the edge, 2 the ray from p to +x crosses it (half-open in y)."""
    straddles = (a[1] <= p[1]) != (b[1] <= p[1])
    in_env = min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])
    if not (straddles or in_env):
        return 0
    o = orientation_exact(a[0], a[1], b[0], b[1], p[0], p[1])
    if o == 0 and in_env:
        return 1
    if straddles:
        up = a[1] <= p[1]
        if (up and o > 0) or (not up and o < 0):
            return 2
    return 0


def is_inside(ring, p) -> bool:
    odd = False
    m = len(ring)
    for j in range(m):
        c = _edge_rule(ring[j], ring[(j + 1) % m], p)
        if c == 1:
            return True
        odd ^= c == 2
    return odd


def refused(ring) -> bool:
    return ring.shape[0] < 3 or not np.isfinite(ring).all()


def pixels_inside(ring, X, Y) -> List[Tuple[int, int]]:
    """(row, col) of the centres inside the ring, row-major."""
    pts = [(float(x), float(y)) for x, y in ring]
    x0, x1, y0, y1 = ring[:, 0].min(), ring[:, 0].max(), ring[:, 1].min(), ring[:, 1].max()
    rr, cc = np.nonzero((X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1))          # exact: beyond its box nothing is inside a ring
    return [(int(r), int(c)) for r, c in zip(rr, cc) if is_inside(pts, (float(X[r, c]), float(Y[r, c])))]


def round_f32(fr: Fraction) -> np.float32:
    """The float32 nearest to an exact rational, ties to even: one rounding."""
    near = np.float32(float(fr))
    best = None
    for c in (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))):
        if np.isfinite(c):
            key = (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1)
            if best is None or key < best[0]:
                best = (key, np.float32(c))
    return best[1]


def crown_row(raster, pix):
    """→ (count, (row, col), [min, max, mean, var] float32) of the raster values at ``pix`` (row-major)."""
    if not pix:
        return 0, (-1, -1), np.full(4, -1.0, np.float32)
    vals = np.array([raster[r, c] for r, c in pix], dtype=np.float32)
    nan = np.flatnonzero(np.isnan(vals))
    if nan.size:
        return len(pix), pix[int(nan[0])], np.full(4, np.nan, np.float32)
    assert np.isfinite(vals).all()
    hi, lo = vals.max(), vals.min()
    k_hi, k_lo = int(np.flatnonzero(vals == hi)[0]), int(np.flatnonzero(vals == lo)[0])
    exact = [Fraction(float(v)) for v in vals]
    mean = sum(exact) / len(exact)
    var = sum((v - mean) ** 2 for v in exact) / len(exact)
    return len(pix), pix[k_hi], np.array([vals[k_lo], vals[k_hi], round_f32(mean), round_f32(var)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(family, i):
    case = cases(family)[i]
    X, Y = centres(case.transform, *case.raster.shape)
    n = len(case.rings)
    status, count = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    pos, stats = np.full((n, 2), -1, np.int32), np.full((n, 4), np.nan, np.float32)
    pix: List[List[Tuple[int, int]]] = []
    for k, ring in enumerate(case.rings):
        if refused(ring):
            status[k] = 2
            pix.append([])
            continue
        pix.append(pixels_inside(ring, X, Y))
        count[k], pos[k], stats[k] = crown_row(case.raster, pix[-1])
    if case.repeat is not None:
        idx = case.repeat
        status, count, pos, stats, pix = status[idx], count[idx], pos[idx], stats[idx], [pix[j] for j in idx]
    return Expected(_frozen(status), _frozen(count), _frozen(pos), _frozen(stats)), pix


def expected(family, i) -> Expected:
    return _oracle(family, i)[0]


def inside(family, i):
    return _oracle(family, i)[1]


def launch_rings(case):
    """The rings a launch sees: the case's, repeated where it says so."""
    return list(case.rings) if case.repeat is None else [case.rings[j] for j in case.repeat]


# ---- the contract, shared by the host and the device tests --------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def selected_differs(got, want):
    """min / max: equal bits, or NaN on both sides (the payload is not part of the contract)."""
    return ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))


def moment_differs(got, want):
    """mean / variance: within one float32 ulp of the exact value rounded once; NaN by class. (Every crafted value is finite or
    NaN.) Why one ulp holds with room: any order of N float64 additions errs by at most (N - 1) * 2^-53 * sum|v|; a crafted crown
    has N <= 2^15 pixels, so the sum is within 2^-38 * sum|v| of exact. Every moment case has values of ONE sign, sum|v| = |sum v|,
    so the float64 mean is within 2^-37 of itself relatively — 2^-13 of a float32 ulp — and lands on the once-rounded float32 or
    its neighbour. The variance sums squares (one sign again) of deviations from that mean: a mean off by delta adds delta^2 exactly
    (the deviations from the true mean sum to zero), and with a spread of at least 2^-10 of the mean, delta^2 <= 2^-74 mean^2 is
    below 2^-54 of the variance. The constant case is exact: N equal float32 values sum exactly in float64, the quotient is the
    value, every deviation is 0."""
    got64, want64 = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(got) & (np.abs(got64 - want64) <= np.spacing(np.abs(want)).astype(np.float64))
    return ~np.where(np.isnan(want), np.isnan(got), near)


def differing(got, want: Expected):
    """got = (stats [n, 4], count [n], max_pos [n, 2], status [n]) → bool [n]: crowns that break the contract."""
    stats, count, pos, status = got
    assert stats.dtype == np.float32 and stats.shape == want.stats.shape and pos.shape == want.pos.shape
    bad = (status != want.status) | (count != want.count) | (pos != want.pos).any(axis=1)
    bad |= selected_differs(stats[:, 0], want.stats[:, 0]) | selected_differs(stats[:, 1], want.stats[:, 1])
    return bad | moment_differs(stats[:, 2], want.stats[:, 2]) | moment_differs(stats[:, 3], want.stats[:, 3])


# ---- boundary -----------------------------------------------------------------------------------------------------------------
def _boundary():
    rows = cols = 12
    t = north_up(rows)
    rings = [rect(2.5, 2.5, 6.5, 6.5),                                  # edges through centres: 5 x 5 inside
             [(1.5, 1.5), (4.5, 1.5), (1.5, 4.5)],                        # vertices on centres, hypotenuse through centres: 4 + 3 + 2 + 1
             [(2.5, 8.5), (9.5, 8.5), (7.2, 10.2), (4.1, 10.2)],          # a horizontal edge along the centre row y = 8.5: 8 + 5 (y = 9.5)
             rect(7.5, 0.5, 11.5, 0.5 + 1e-12)]                           # nearly flat, its lower edge on the row y = 0.5: 5
    return [_case("on_centres", distinct(rows, cols, 11), t, rings, counts=[25, 10, 13, 5])]


# ---- scanline -----------------------------------------------------------------------------------------------------------------
def _scanline():
    rows = cols = 12
    t = north_up(rows)
    diamond = [(5.5, 2.5), (8.5, 5.5), (5.5, 8.5), (2.5, 5.5)]            # |dx| + |dy| <= 3 on the centres: 25
    # spikes from below up to the centre row y = 5.5: apex ON the centre (5.5, 5.5) and BETWEEN two centres at x = 9.0
    spikes = [(1.2, 1.2), (10.8, 1.2), (10.8, 3.2), (9.25, 3.2), (9.0, 5.5), (8.75, 3.2), (6.0, 3.2), (5.5, 5.5), (5.0, 3.2), (1.2, 3.2)]
    # a notch from above down to the centre row y = 6.5, its tip between two centres: both of its edges cross the ray, and cancel
    notch = [(1.2, 6.5 - 3.3), (10.8, 6.5 - 3.3), (10.8, 9.8), (6.3, 9.8), (6.0, 6.5), (5.7, 9.8), (1.2, 9.8)]
    collinear = [(2.5, 2.5), (4.0, 2.5), (4.5, 2.5), (7.5, 2.5), (7.5, 5.5), (2.5, 5.5)]     # extra vertices on a centre row: 6 x 4
    return [_case("vertices_on_rows", distinct(rows, cols, 12), t, [diamond, spikes, notch, collinear], counts=[25, 23, None, 24],
                  alone_on_row={1: (5.5, 5.5)})]


# ---- concave / winding --------------------------------------------------------------------------------------------------------
U_RING = [(1.2, 1.2), (10.8, 1.2), (10.8, 9.8), (7.8, 9.8), (7.8, 4.2), (4.2, 4.2), (4.2, 9.8), (1.2, 9.8)]
COMB = [(1.2, 11.2), (14.8, 11.2), (14.8, 14.8), (12.2, 14.8), (12.2, 12.8), (9.8, 12.8), (9.8, 14.8), (7.2, 14.8), (7.2, 12.8), (4.8, 12.8),
        (4.8, 14.8), (1.2, 14.8)]
NOTCHES = {0: [(16 - 7, 5), (16 - 7, 6)], 1: [(16 - 14, 5), (16 - 14, 11)]}       # (row, col) in the notches: y = 6.5 / 13.5


def _concave_raster():
    raster = distinct(16, 16, 13)
    for pix in NOTCHES.values():
        for r, c in pix:
            raster[r, c] = 9.0                                            # the largest values lie in the notches
    return raster


def _concave():
    return [_case("u_and_comb", _concave_raster(), north_up(16), [U_RING, COMB], notches=NOTCHES)]


def _winding():
    bowtie = [(1.5, 1.5), (8.5, 8.5), (8.5, 1.5), (1.5, 8.5)]
    penta = [(8.0 + 6.5 * math.sin(4 * math.pi * k / 5), 8.0 + 6.5 * math.cos(4 * math.pi * k / 5)) for k in range(5)]
    return [_case("reversed", _concave_raster(), north_up(16), [U_RING, U_RING[::-1], COMB, COMB[::-1], U_RING[3:] + U_RING[:3]],
                  groups=[[0, 1, 4], [2, 3]]),
            _case("self_crossing", distinct(16, 16, 14), north_up(16), [bowtie, bowtie[::-1], penta], groups=[[0, 1]],
                  outside={2: (16 - 8, 7)})]                               # the pentagram's core (x 7.5, y 7.5): wound twice, even


# ---- clipping -----------------------------------------------------------------------------------------------------------------
def _clipping():
    rows, cols = 9, 11
    t = north_up(rows)
    r = []
    r += [rect(-3.3, 2.2, 2.2, 5.2), rect(8.7, 2.2, 14.1, 5.2), rect(4.2, 6.7, 7.2, 12.0), rect(4.2, -4.0, 7.2, 2.1)]     # each side
    r += [rect(-2.0, 6.6, 2.1, 11.0), rect(8.9, 6.6, 13.0, 11.0), rect(-2.0, -2.0, 2.1, 2.3), rect(8.9, -2.0, 13.0, 2.3)]  # each corner
    r += [rect(-9.0, 2.0, -1.2, 5.0), rect(12.2, 2.0, 20.0, 5.0), rect(3.0, 10.1, 6.0, 15.0), rect(3.0, -8.0, 6.0, -0.6), rect(1e7, 1e7, 1e7 + 5, 1e7 + 5)]
    r += [rect(3.6, 1.0, 3.9, 8.0), rect(1.0, 4.6, 10.0, 4.9), rect(4.6, 4.6, 4.9, 4.9)]                                   # slivers between centres
    r += [rect(-50.0, -50.0, 50.0, 50.0)]                                                                                   # larger than the raster
    out = [_case("9x11", distinct(rows, cols, 15), t, r, empty=list(range(8, 16)), counts={16: rows * cols})]
    one = np.array([[0.625]], np.float32)
    out.append(_case("1x1", one, north_up(1), [rect(0.2, 0.2, 0.8, 0.8), rect(0.5, 0.5, 3.0, 3.0), rect(0.6, 0.2, 0.9, 0.8), rect(-5.0, -5.0, 5.0, 5.0)],
                     empty=[2], counts={0: 1, 1: 1, 3: 1}))
    return out


# ---- large coordinates --------------------------------------------------------------------------------------------------------
def _large():
    rows = cols = 24
    t = (0.2, 0.0, UTM_X, 0.0, -0.2, UTM_Y)
    X, Y = centres(t, rows, cols)
    rng = np.random.default_rng(16)
    rings = [star(rng, X[r, c] + rng.uniform(-0.1, 0.1), Y[r, c] + rng.uniform(-0.1, 0.1), 0.3, 1.4, int(m))
             for r, c, m in zip(rng.integers(2, 22, 12), rng.integers(2, 22, 12), rng.integers(5, 25, 12))]
    # (ring, edge, (row, col), kind): what the rational orientation of the centre against the edge must be — "zero", "nonzero", or
    # "tiny": not zero, yet below 1e-15 of the products it is the difference of, where only the double-double path decides
    near = []
    # exactly through a centre: the diagonal of a square around (12, 12) — the centre is ON it
    qx, qy = float(X[12, 12]), float(Y[12, 12])
    rings.append(np.array([(qx - 1.0, qy - 1.0), (qx + 1.0, qy + 1.0), (qx - 1.0, qy + 1.0)]))
    near.append((len(rings) - 1, 0, (12, 12), "zero"))
    # one unit in the last place of y off a row of centres: the edge starts above row 5's centres and ends below them
    y5 = float(Y[5, 0])
    rings.append(np.array([(float(X[5, 2]) - 0.05, y5 + UY), (float(X[5, 20]) + 0.05, y5 - UY), (float(X[5, 20]) + 0.05, y5 + 0.9),
                           (float(X[5, 2]) - 0.05, y5 + 0.9)]))
    near += [(len(rings) - 1, 0, (5, 3), "nonzero"), (len(rings) - 1, 0, (5, 19), "nonzero")]
    # a determinant of 2^-61 against the centre of (17, 6): far below the filter's bound 1e-15 * (|products|), not zero
    qx, qy = float(X[17, 6]), float(Y[17, 6])
    ax, ay = qx - 1.0 + 8 * UX, qy - 1.0
    rings.append(np.array([(ax, ay), (ax + 2.0, ay + 2.0 + UY), (ax - 0.5, ay + 2.5)]))
    near.append((len(rings) - 1, 0, (17, 6), "tiny"))
    rings.append(np.array([(ax, ay), (ax + 2.0, ay + 2.0 + UY), (ax + 2.5, ay - 0.5)]))      # the same edge, the ring on its other side
    near.append((len(rings) - 1, 0, (17, 6), "tiny"))
    return [_case("utm_0.2m", distinct(rows, cols, 16), t, rings, near=near)]


# ---- transforms ---------------------------------------------------------------------------------------------------------------
def _transforms():
    rows, cols = 20, 24
    s, th = 0.5, math.radians(4.0)
    transforms = {
        "south_up": (0.5, 0.0, 1000.0, 0.0, 0.5, 2000.0),
        "west_positive": (-0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0),
        "south_up_west_positive": (-0.5, 0.0, 1000.0, 0.0, 0.5, 2000.0),
        "anisotropic": (0.5, 0.0, 1000.0, 0.0, -0.2, 2000.0),
        "rotated": (s * math.cos(th), s * math.sin(th), 1000.0, s * math.sin(th), -s * math.cos(th), 2000.0),
    }
    raster = distinct(rows, cols, 17)
    out = []
    for j, (name, t) in enumerate(transforms.items()):
        rng = np.random.default_rng(170 + j)
        X, Y = centres(t, rows, cols)
        rr = np.concatenate([[0, rows - 1, rows // 2], rng.integers(0, rows, 7)])
        cc = np.concatenate([[0, cols - 1, cols // 2], rng.integers(0, cols, 7)])
        rings = [star(rng, X[r, c], Y[r, c], 0.4, 2.5, int(rng.integers(4, 14))) for r, c in zip(rr, cc)]
        # and a quadrilateral with vertices ON four centres, so that edges run through centres under this transform too
        rings.append(np.array([(X[4, 5], Y[4, 5]), (X[4, 15], Y[4, 15]), (X[14, 15], Y[14, 15]), (X[14, 5], Y[14, 5])]))
        out.append(_case(name, raster, t, rings))
    return out


# ---- values -------------------------------------------------------------------------------------------------------------------
NAN_CROWNS = ("one", "several", "first", "last", "all", "notch_only")


def _values():
    rows, cols = 26, 40
    t = north_up(rows)
    X, Y = centres(t, rows, cols)
    squares = [rect(1.2 + 8 * k, 14.2, 7.8 + 8 * k, 24.8) for k in range(5)]               # 7 x 11 centres each
    u = [(1.2, 1.2), (12.8, 1.2), (12.8, 11.8), (9.8, 11.8), (9.8, 4.2), (4.2, 4.2), (4.2, 11.8), (1.2, 11.8)]
    rings = squares + [u]
    pix = [pixels_inside(np.array(r), X, Y) for r in rings]
    out = []
    raster = distinct(rows, cols, 18)
    hits = []
    for k, what in enumerate(NAN_CROWNS):
        p = pix[k]
        if what == "one":
            hit = [p[len(p) // 2]]
        elif what == "several":
            hit = [p[3], p[len(p) // 5], p[len(p) // 2 + 1], p[-9]]
        elif what == "first":
            hit = [p[0]]
        elif what == "last":
            hit = [p[-1]]
        elif what == "all":
            hit = p
        else:                                                             # every pixel of the U's box that the U leaves out
            box = {(r, c) for r in range(rows) for c in range(cols) if 1.2 <= X[r, c] <= 12.8 and 1.2 <= Y[r, c] <= 11.8}
            hit = sorted(box - set(p))
            assert hit
        for r, c in hit:
            raster[r, c] = np.nan
        hits.append(len(hit))
    out.append(_case("nan", raster, t, rings, nan_crowns=[0, 1, 2, 3, 4], clean_crowns=[5], hits=hits))

    rng = np.random.default_rng(19)
    quantised = rng.integers(0, 4, (rows, cols)).astype(np.float32)
    out.append(_case("quantised", quantised, t, rings))
    placed = quantised.copy()
    for k, where in enumerate(([0, 30, -5], [-2, -1], [10, 11], [0, -1])):       # equal maxima: first and later, last two, neighbours, both ends
        for j in where:
            placed[pix[k][j]] = 9.0
    out.append(_case("placed", placed, t, rings, first_max={0: pix[0][0], 1: pix[1][-2], 2: pix[2][10], 3: pix[3][0]}))
    # zeros of both signs over negative values: maximum a zero with the sign of the FIRST zero inside; and over positive values: minimum
    for name, sign in (("zero_max", -1.0), ("zero_min", 1.0)):
        zeros = sign * (1.0 + rng.integers(0, 3, (rows, cols))).astype(np.float32)
        is_zero = rng.random((rows, cols)) < 0.3
        zeros[is_zero] = np.where(rng.random(int(is_zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        for k, z in enumerate((-0.0, 0.0, -0.0, 0.0, -0.0, 0.0)):
            zeros[pix[k][0]] = z
        out.append(_case(name, zeros, t, rings, first_zero_negative=[True, False, True, False, True, False], which=1 if sign < 0 else 0))
    out.append(_case("constant", np.full((rows, cols), 0.37, np.float32), t, rings, constant=0.37))
    return out


# ---- lanes --------------------------------------------------------------------------------------------------------------------
def _lanes():
    out = []
    rows, cols = 8, 140
    t = north_up(rows)
    rings = [rect(3.2 + k, 1.2 + (k % 3), 3.2 + k + w - 0.4, 3.8 + (k % 3)) for k, w in enumerate((1, 63, 64, 65, 129))]      # 3 rows of w centres
    rings.append(rect(2.2, 6.2, 131.8, 6.8))                                                      # one row tall, 130 wide
    rings.append([(1.2, 0.2), (138.8, 0.2), (138.8, 7.8), (70.0, 1.0), (1.2, 7.8)])               # a wide V: two runs on most rows
    out.append(_case("widths", distinct(rows, cols, 20), t, rings, counts=[3, 189, 192, 195, 387, 130, None]))
    out.append(_case("one_column", distinct(140, 5, 21), north_up(140), [rect(2.2, 4.2, 2.8, 134.8), rect(0.1, 0.1, 4.9, 139.9)], counts=[131, 700]))
    # more runs of 64 pixels than the kernel keeps verdicts for (140 rows x 3 runs): its second pass walks again
    out.append(_case("many_runs", distinct(140, 140, 24), north_up(140), [rect(0.2, 0.2, 139.8, 139.8), [(0.2, 0.2), (139.8, 0.2), (70.0, 139.8)]],
                     counts=[19600, None]))
    # 300 small crowns of one size at scattered places, then duplicates: repeated until the launch has more crowns than it holds in flight
    rows = cols = 40
    rng = np.random.default_rng(22)
    base = []
    for k in range(300):
        cx, cy = rng.uniform(1, 39, 2)
        base.append(np.array([(cx - 1.3, cy - 1.1), (cx + 1.4, cy - 1.2), (cx + 1.2, cy + 1.3), (cx - 1.1, cy + 1.2)]))
    repeat = np.concatenate([np.arange(300), rng.integers(0, 300, IN_FLIGHT + 77 - 300)])
    out.append(_case("grid_stride", distinct(rows, cols, 22), north_up(rows), base, repeat=_frozen(repeat)))
    return out


# ---- capacity -----------------------------------------------------------------------------------------------------------------
def regular(m, cx=8.0, cy=8.0, r=6.3):
    k = np.arange(m)
    return np.stack([cx + r * np.cos(2 * np.pi * k / m), cy + r * np.sin(2 * np.pi * k / m)], axis=1)


def _capacity():
    good = rect(2.2, 2.2, 6.8, 5.8)
    rings = [good, regular(RING_CAP), np.zeros((0, 2)), regular(RING_CAP + 1), [(1.0, 1.0)], good, [(1.0, 1.0), (5.0, 5.0)],
             [(1.0, 1.0), (np.nan, 5.0), (1.0, 9.0)], regular(RING_CAP, 7.5, 7.5, 5.0), [(1.0, 1.0), (9.0, 1.0), (np.inf, 9.0)],
             regular(3 * RING_CAP, 7.5, 7.5, 5.0), good]
    return [_case("at_and_over", distinct(16, 16, 23), north_up(16), rings, over=[3, 10], refused=[2, 4, 6, 7, 9], groups=[[0, 5, 11]])]


FAMILIES = {"boundary": _boundary, "scanline": _scanline, "concave": _concave, "winding": _winding, "clipping": _clipping, "large": _large,
            "transforms": _transforms, "values": _values, "lanes": _lanes, "capacity": _capacity}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(FAMILIES[family]())
