"""Shared inputs of the crown-statistics tests (test_crown_cases.py, test_crown_stats_gpu.py): crafted rasters and circles for
td_crown_stats, and what oracle.postprocess_ref makes of them. Not a test; pure numpy.

``cases(family)`` → a tuple of :class:`Case` (raster float32 [rows, cols], transform 6-tuple, bounds, circles float32 [n, 3], mode,
radius_scale, then a name and the facts test_crown_cases.py verifies with the oracle alone). ``expected(family, i)`` → the oracle's
result for case ``i``, computed once and read-only: [n, 3] (max, x, y) in height mode (0), [n, 4] (min, max, mean, var) in NDVI mode
(1). The oracle takes vertex arrays, not circles: :func:`vertices` gives the two ends of the horizontal diameter and the centre, and
every circle here lies on a grid on which ``cx - r`` and ``cx + r`` are float32 values, so that the oracle's ``_circle`` returns
(cx, cy, r) bit for bit.

  f32_rounding    UTM coordinates (412 000 / 5 318 060) at 0.05 m and 0.02 m pixels: a float32 step is 0.5 m in y there, so the float32
                  membership test of NDVI mode takes in whole rows far outside the circle; a height-mode twin of the same geometry
  nan_pixels      one, several, first, last, every inside pixel NaN; NaNs on and off the 256-thread stride of the kernel's box
                  traversal; a ring of NaNs just outside the circle
  ties            (height) plateaus: quantised values on circles of more than 1 024 pixels, equal maxima at the first and at the last
                  inside pixels, a later equal maximum on a lower thread, a constant raster, +0.0 against -0.0
  extremes        +-inf, all -inf, denormals; (NDVI) a constant raster and a large mean with a tiny spread
  boundary        integer geometry with the maximum exactly ON the circle (3-4-5, 5-12-13) or on the nearest pixel outside; r = 0
  clipping        circles cut by every edge and corner of 37 x 301 and 301 x 37 rasters, outside them (near and 1e7 m away), larger
                  than the raster, holding one pixel
  orientation     south-up, west-positive, both, rotated by four degrees, anisotropic pixels
  windows         bounds smaller than the raster with r_lo != c_lo (the reference adds the ROW offset to the COLUMN index and vice
                  versa), one row, one column
  scale_and_grid  radius_scale 0.3 and 0.7, one crown, 300 crowns, duplicated crowns
"""
import functools
import math
import warnings
from typing import Any, Dict, NamedTuple, Tuple

import numpy as np

from oracle import postprocess_ref as O

HEIGHT, NDVI = 0, 1
UTM_X, UTM_Y = 412000.0, 5318060.0


class Case(NamedTuple):
    raster: np.ndarray
    transform: Tuple[float, float, float, float, float, float]
    bounds: Tuple[float, float, float, float]
    circles: np.ndarray
    mode: int
    radius_scale: float
    name: str
    facts: Dict[str, Any]


def _frozen(a):
    a.setflags(write=False)
    return a


def _case(name, raster, transform, bounds, circles, mode, radius_scale=1.0, **facts):
    raster = _frozen(np.ascontiguousarray(raster, dtype=np.float32))
    circles = _frozen(np.ascontiguousarray(circles, dtype=np.float32).reshape(-1, 3))
    assert raster.shape[0] <= 400 and raster.shape[1] <= 400
    return Case(raster, tuple(float(v) for v in transform), tuple(float(v) for v in bounds), circles, mode, float(radius_scale),
                f"{name}/{'ndvi' if mode else 'height'}", facts)


def distinct(rows, cols, seed, lo=-1.0, hi=1.0):
    """float32 [rows, cols] whose values all differ (a seeded permutation of an even grid over (lo, hi)): a pixel missed or taken
    in wrongly moves the minimum, the maximum or the mean."""
    n = rows * cols
    p = np.random.default_rng(seed).permutation(n).astype(np.float64)
    out = (lo + (hi - lo) * (p + 0.5) / n).astype(np.float32).reshape(rows, cols)
    assert np.unique(out).size == n
    return out


def full_bounds(transform, rows, cols):
    """(minx, miny, maxx, maxy) that the reference's window arithmetic (a and e only) turns into the whole raster."""
    a, _, c, _, e, f = transform
    xs, ys = (c, c + a * cols), (f, f + e * rows)
    return min(xs), min(ys), max(xs), max(ys)


def vertices(circles):
    """→ (list of x arrays, list of y arrays), float32: per circle the ends of its horizontal diameter and its centre."""
    c = np.asarray(circles, dtype=np.float32).reshape(-1, 3)
    px = [np.array([cx - r, cx + r, cx], dtype=np.float32) for cx, _, r in c]
    py = [np.array([cy, cy, cy], dtype=np.float32) for _, cy, _ in c]
    return px, py


def window(case):
    """(r_lo, c_lo, sub_rows, sub_cols) of the reference's subset for the case's bounds."""
    sub, r_lo, c_lo = O._subset(case.raster, case.transform, case.raster.shape[0], case.raster.shape[1], case.bounds)
    return r_lo, c_lo, sub.shape[0], sub.shape[1]


def inside_masks(case):
    """→ (masks bool [n, subset pixels], xs float64, ys float64, flattened subset): the membership test of heights_within /
    ndvi_within written out with the oracle's own helpers (test_crown_cases.py checks it against their results)."""
    sub, r_lo, c_lo = O._subset(case.raster, case.transform, case.raster.shape[0], case.raster.shape[1], case.bounds)
    xs, ys = O._pixel_coords(sub.shape, case.transform, r_lo, c_lo)
    tx, ty = (xs.astype(np.float32), ys.astype(np.float32)) if case.mode == NDVI else (xs, ys)
    masks = np.zeros((case.circles.shape[0], xs.size), bool)
    with np.errstate(all="ignore"):
        for i, (px, py) in enumerate(zip(*vertices(case.circles))):
            cx, cy, rad = O._circle(px, py)
            if case.mode == NDVI:
                rad = rad * np.float32(case.radius_scale)
            masks[i] = (tx - cx) ** 2 + (ty - cy) ** 2 <= rad ** 2
    return masks, xs, ys, sub.flatten()


def kernel_box(case, k):
    """(r0, c0, bh, bw) in subset indices: the box crown_stats_kernel (crown.hip) walks for crown ``k``, thread ``p % 256`` taking
    the box's p-th pixel in row-major order. A model of the kernel's traversal, used ONLY to aim values at particular threads (a NaN
    a multiple of 256 after the box origin, a later tie on a lower thread); no expected value depends on it."""
    a, b, c, d, e, f = case.transform
    r_lo, c_lo, sub_rows, sub_cols = window(case)
    if not (b == 0.0 and d == 0.0 and a != 0.0 and e != 0.0):
        return 0, 0, sub_rows, sub_cols
    cx, cy = float(case.circles[k, 0]), float(case.circles[k, 1])
    r = float(np.float32(case.circles[k, 2]) * np.float32(case.radius_scale))
    mx = my = r * 1.0001 + 1e-3
    if case.mode == NDVI:
        mx += max(abs(a * r_lo + c), abs(a * (r_lo + sub_cols - 1) + c)) * 2.0 ** -24
        my += max(abs(e * c_lo + f), abs(e * (c_lo + sub_rows - 1) + f)) * 2.0 ** -24
    u0, u1 = sorted(((cx - mx - c) / a, (cx + mx - c) / a))
    v0, v1 = sorted(((cy - my - f) / e, (cy + my - f) / e))
    c0, c1 = max(math.floor(u0) - 1 - r_lo, 0), min(math.ceil(u1) + 1 - r_lo, sub_cols - 1)
    r0, r1 = max(math.floor(v0) - 1 - c_lo, 0), min(math.ceil(v1) + 1 - c_lo, sub_rows - 1)
    return r0, c0, r1 - r0 + 1, c1 - c0 + 1


def box_position(case, k, lin):
    """Row-major position inside crown k's box of the subset pixel with flattened subset index ``lin`` (None outside the box)."""
    r0, c0, bh, bw = kernel_box(case, k)
    sub_cols = window(case)[3]
    rs, cs = lin // sub_cols - r0, lin % sub_cols - c0
    return rs * bw + cs if 0 <= rs < bh and 0 <= cs < bw else None


# ---- f32_rounding -------------------------------------------------------------------------------------------------------------
def _utm_circles(rng, n, rows, cols, pixel, k_lo, k_hi):
    """n circles on a north-up raster at UTM_X / UTM_Y: radii k / 32 m, cx on the 1 / 32 m grid of float32 there, cy on its 0.5 m grid."""
    r = rng.integers(k_lo, k_hi + 1, n) / 32.0
    cx = UTM_X + rng.integers(0, int(cols * pixel * 32) + 1, n) / 32.0
    cy = UTM_Y - rng.integers(0, int(rows * pixel * 2) + 1, n) / 2.0
    return np.stack([cx, cy, r], axis=1)


def _f32_rounding():
    out = []
    for pixel, seed in ((0.05, 50), (0.02, 20)):
        t = (pixel, 0.0, UTM_X, 0.0, -pixel, UTM_Y)
        raster = distinct(400, 400, seed)
        # 3 to 30 pixels of radius in steps of 1 / 32 m
        circles = _utm_circles(np.random.default_rng(seed), 64, 400, 400, pixel, math.ceil(3 * pixel * 32), math.floor(30 * pixel * 32))
        b = full_bounds(t, 400, 400)
        for scale in (1.0, 0.5):
            out.append(_case(f"utm_{pixel}m_scale{scale}", raster, t, b, circles, NDVI, scale, pixel=pixel))
        out.append(_case(f"utm_{pixel}m", raster, t, b, circles, HEIGHT, 1.0, pixel=pixel))
    return out


# ---- nan_pixels ---------------------------------------------------------------------------------------------------------------
NAN_CROWNS = ("one", "several", "first", "last", "stride", "off_stride", "all", "ring_outside")


def _nan_pixels():
    out = []
    rows, cols = 120, 160
    t = (1.0, 0.0, 0.0, 0.0, -1.0, float(rows))                       # x = col, y = rows - row
    circles = np.array([[20 + 40 * (k % 4), rows - (30 + 60 * (k // 4)), 12.25] for k in range(8)])
    b = full_bounds(t, rows, cols)
    for mode in (HEIGHT, NDVI):
        base = distinct(rows, cols, 7)
        probe = _case("nan", base, t, b, circles, mode)
        masks = inside_masks(probe)[0]
        flat = base.flatten()
        counts = []
        for k, what in enumerate(NAN_CROWNS):
            idx = np.flatnonzero(masks[k])
            pos = np.array([box_position(probe, k, int(i)) for i in idx])
            assert idx.size > 256 and (pos >= 0).all()
            if what == "one":
                hit = idx[[idx.size // 2]]
            elif what == "several":
                hit = idx[[3, idx.size // 5, idx.size // 3, idx.size // 2 + 1, idx.size - 9]]
            elif what == "first":
                hit = idx[[0]]
            elif what == "last":
                hit = idx[[-1]]
            elif what == "stride":
                hit = idx[(pos % 256 == 0) & (pos > 0)][:1]
            elif what == "off_stride":
                hit = idx[pos % 256 == 37][-1:]
            elif what == "all":
                hit = idx
            else:                                                     # every pixel of the box that the circle leaves out
                r0, c0, bh, bw = kernel_box(probe, k)
                box = (np.arange(r0, r0 + bh)[:, None] * cols + np.arange(c0, c0 + bw)[None, :]).flatten()
                flat[np.setdiff1d(box, idx)] = np.nan
                hit = idx[:0]
            assert what == "ring_outside" or hit.size
            flat[hit] = np.nan
            counts.append(int(hit.size))
        out.append(_case("nan", flat.reshape(rows, cols), t, b, circles, mode, nan_inside=counts))
    return out


# ---- ties ---------------------------------------------------------------------------------------------------------------------
def _ties():
    rows, cols = 96, 200
    t = (1.0, 0.0, 0.0, 0.0, -1.0, float(rows))
    b = full_bounds(t, rows, cols)
    four = np.array([[25 + 50 * k, rows - 48, 20.0 + 0.25 * k] for k in range(4)])        # disjoint, 1 257 pixels and more each
    rng = np.random.default_rng(31)
    out = []
    quantised = rng.integers(0, 4, (rows, cols)).astype(np.float32)
    overlapping = np.array([[40, 50, 19.5], [55, 44, 25.0], [120, 48, 30.0], [150, 60, 22.75]])
    out.append(_case("quantised", quantised, t, b, overlapping, HEIGHT))

    # crown 0: the maximum on the first inside pixel and twice more; crown 1: only on the last two inside pixels; crown 2: twice,
    # the later one on a lower thread; crown 3: twice on one thread (256 box positions apart) and once more in between
    probe = _case("placed", quantised, t, b, four, HEIGHT)
    masks = inside_masks(probe)[0]
    flat = quantised.flatten()
    placed = []
    for k in range(4):
        idx = np.flatnonzero(masks[k])
        pos = np.array([box_position(probe, k, int(i)) for i in idx])
        if k == 0:
            hit = idx[[0, idx.size // 2, idx.size - 5]]
        elif k == 1:
            hit = idx[-2:]
        elif k == 2:
            first = int(np.flatnonzero(pos % 256 == 250)[0])
            later = first + int(np.flatnonzero(pos[first:] % 256 == 2)[0])
            hit = idx[[first, later]]
        else:
            pairs = np.flatnonzero(np.isin(pos + 256, pos))                 # inside pixels with an inside pixel one stride later
            first = int(pairs[pairs.size // 2])
            same = int(np.flatnonzero(pos == pos[first] + 256)[0])
            hit = idx[[first, (first + same) // 2, same]]
        flat[hit] = 9.0
        placed.append([int(i) for i in hit])
    out.append(_case("placed", flat.reshape(rows, cols), t, b, four, HEIGHT, placed=placed))

    out.append(_case("constant", np.full((rows, cols), 2.5, np.float32), t, b, four, HEIGHT))

    # zeros of both signs over negative values: the maximum is a zero, and its sign is the sign of the FIRST zero inside
    zeros = -1.0 - rng.integers(0, 3, (rows, cols)).astype(np.float32)
    is_zero = rng.random((rows, cols)) < 0.3
    zeros[is_zero] = np.where(rng.random(int(is_zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    probe = _case("signed_zero", zeros, t, b, four, HEIGHT)
    masks = inside_masks(probe)[0]
    flat = zeros.flatten()
    for k, z in enumerate((-0.0, 0.0, -0.0, 0.0)):
        flat[np.flatnonzero(masks[k])[0]] = z
    out.append(_case("signed_zero", flat.reshape(rows, cols), t, b, four, HEIGHT))
    return out


# ---- extremes -----------------------------------------------------------------------------------------------------------------
def _extremes():
    rows, cols = 64, 128
    t = (1.0, 0.0, 0.0, 0.0, -1.0, float(rows))
    b = full_bounds(t, rows, cols)
    # -inf at (row 32, col 20), +inf at (row 32, col 100): crown 0 holds only the first, crown 1 only the second, crown 2 both
    circles = np.array([[20, 32, 6.0], [100, 32, 6.0], [60, 32, 45.0], [64, 30, 20.5]])
    infs = distinct(rows, cols, 41, -50.0, 50.0)
    infs[32, 20], infs[32, 100] = -np.inf, np.inf
    denormal = _frozen((np.random.default_rng(43).permutation(rows * cols) + 1).astype(np.uint32).view(np.float32).reshape(rows, cols))
    spread = (1000.0 + np.random.default_rng(44).integers(0, 64, (rows, cols)) * 2.0 ** -13).astype(np.float32)
    out = []
    for mode in (HEIGHT, NDVI):
        out.append(_case("infinities", infs, t, b, circles, mode))
        out.append(_case("all_minus_inf", np.full((rows, cols), -np.inf, np.float32), t, b, circles, mode))
        out.append(_case("denormals", denormal, t, b, circles, mode))
    out.append(_case("constant", np.full((rows, cols), 0.37, np.float32), t, b, circles, NDVI, constant=0.37))
    out.append(_case("large_mean_tiny_spread", spread, t, b, circles, NDVI))
    return out


# ---- boundary -----------------------------------------------------------------------------------------------------------------
def _boundary():
    rows, cols = 48, 170
    t = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0)                                # x = col, y = -row
    b = full_bounds(t, rows, cols)
    # crowns 0 / 2: the raster's maximum lies ON the circle (3-4-5, 5-12-13); crowns 1 / 3: on the nearest pixel outside (distance^2
    # r^2 + 1); crown 4: r = 0 on a pixel position; crowns 5 / 6: r = 0 between positions
    circles = np.array([[20, -24, 5], [50, -24, 5], [90, -24, 13], [135, -24, 13], [160, -10, 0], [160.5, -10, 0], [160, -10.5, 0]])
    on = {0: (3, 4), 2: (5, 12)}
    off = {1: (5, 1), 3: (13, 1)}
    raster = distinct(rows, cols, 51, 0.0, 1.0)
    marks = {}
    for k, (dx, dy) in {**on, **off}.items():
        col, row = int(circles[k, 0]) + dx, -(int(circles[k, 1]) + dy)
        raster[row, col] = 5.0
        marks[k] = (row, col)
    return [_case("integer", raster, t, b, circles, mode, on_circle={k: marks[k] for k in on}, just_outside={k: marks[k] for k in off})
            for mode in (HEIGHT, NDVI)]


# ---- clipping -----------------------------------------------------------------------------------------------------------------
def _clipping():
    out = []
    for rows, cols in ((37, 301), (301, 37)):
        t = (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)
        x0, x1, y1, y0 = 1000.0, 1000.0 + 0.5 * (cols - 1), 2000.0, 2000.0 - 0.5 * (rows - 1)      # first / last pixel positions
        xm, ym = 1000.0 + 0.5 * (cols // 2), 2000.0 - 0.5 * (rows // 2)
        r = 4.0
        c = [(x0 + 1, ym, r), (x1 - 1, ym, r), (xm, y1 - 1, r), (xm, y0 + 1, r)]                    # cut by one edge
        c += [(x0 + 1, y1 - 1, r), (x1 - 1, y1 - 1, r), (x0 + 1, y0 + 1, r), (x1 - 1, y0 + 1, r)]    # by a corner
        c += [(x0 - r - 0.25, ym, r), (x1 + r + 0.25, ym, r), (xm, y1 + r + 0.25, r), (xm, y0 - r - 0.25, r)]   # outside, a quarter metre short
        c += [(x0 - 20, ym, r), (x1 + 20, ym, r), (xm, y1 + 20, r), (xm, y0 - 20, r)]               # outside, box and all
        c += [(x0 - 1e7, ym, r), (x0 + 1e7, ym, r), (xm, y1 + 1e7, r), (xm, y1 - 1e7, r)]            # 1e7 m away
        c += [(xm, ym, 256.0)]                                                                        # larger than the raster
        c += [(x0 + 5.0, y1 - 2.5, 0.125)]                                                            # one pixel
        raster = distinct(rows, cols, rows)
        for mode in (HEIGHT, NDVI):
            out.append(_case(f"{rows}x{cols}", raster, t, full_bounds(t, rows, cols), np.array(c), mode, empty=list(range(8, 20)), single=21))
    return out


# ---- orientation --------------------------------------------------------------------------------------------------------------
def _orientation():
    rows, cols = 80, 96
    s, th = 0.5, math.radians(4.0)
    transforms = {
        "south_up": (0.5, 0.0, 1000.0, 0.0, 0.5, 2000.0),
        "west_positive": (-0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0),
        "south_up_west_positive": (-0.5, 0.0, 1000.0, 0.0, 0.5, 2000.0),
        "rotated": (s * math.cos(th), s * math.sin(th), 1000.0, s * math.sin(th), -s * math.cos(th), 2000.0),
        "anisotropic": (0.5, 0.0, 1000.0, 0.0, -0.2, 2000.0),
    }
    raster = distinct(rows, cols, 61)
    out = []
    for j, (name, t) in enumerate(transforms.items()):
        rng = np.random.default_rng(600 + j)
        a, b, c, d, e, f = t
        rr = np.concatenate([[0, rows - 1, rows // 2], rng.integers(0, rows, 9)])
        cc = np.concatenate([[0, cols - 1, cols // 2], rng.integers(0, cols, 9)])
        cx = np.round((a * cc + b * rr + c) * 64) / 64                  # circles on a 1 / 64 m grid around pixel positions
        cy = np.round((d * cc + e * rr + f) * 64) / 64
        r = rng.integers(16, 640, rr.size) / 64.0
        for mode in (HEIGHT, NDVI):
            out.append(_case(name, raster, t, full_bounds(t, rows, cols), np.stack([cx, cy, r], axis=1), mode))
    return out


# ---- windows ------------------------------------------------------------------------------------------------------------------
def _windows():
    rows, cols = 60, 140
    t = (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)
    raster = distinct(rows, cols, 71)

    def bounds(r_lo, c_lo, r_hi, c_hi):
        return 1000.0 + 0.5 * c_lo, 2000.0 - 0.5 * r_hi, 1000.0 + 0.5 * c_hi, 2000.0 - 0.5 * r_lo

    out = []
    for name, win in (("window", (7, 23, 40, 110)), ("one_row", (12, 5, 12, 100)), ("one_column", (3, 30, 50, 30))):
        b = bounds(*win)
        for mode in (HEIGHT, NDVI):
            probe = _case(name, raster, t, b, np.zeros((1, 3)), mode)
            assert window(probe) == (win[0], win[1], win[2] - win[0] + 1, win[3] - win[1] + 1)
            xs, ys = O._pixel_coords(window(probe)[2:], t, win[0], win[1])       # where the reference believes the subset's pixels lie
            rng = np.random.default_rng(700 + len(out))
            pick = rng.integers(0, xs.size, 14)
            cx = xs[pick] + rng.integers(-3, 4, pick.size) / 4.0
            cy = ys[pick] + rng.integers(-3, 4, pick.size) / 4.0
            r = rng.integers(1, 25, pick.size) / 4.0
            far = [[xs.min() - 30.0, ys.min(), 2.0], [xs.max(), ys.max() + 30.0, 2.0]]
            out.append(_case(name, raster, t, b, np.concatenate([np.stack([cx, cy, r], axis=1), far]), mode, window=win))
    return out


# ---- scale_and_grid -----------------------------------------------------------------------------------------------------------
def _scale_and_grid():
    out = []
    rows, cols = 150, 130
    t = (0.2, 0.0, UTM_X, 0.0, -0.2, UTM_Y)
    raster = distinct(rows, cols, 81)
    circles = _utm_circles(np.random.default_rng(81), 24, rows, cols, 0.2, 32, 160)        # 1 to 5 m
    for scale in (0.3, 0.7):
        out.append(_case(f"scale{scale}", raster, t, full_bounds(t, rows, cols), circles, NDVI, scale))
    rows = cols = 200
    t = (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)
    raster = distinct(rows, cols, 82)
    rng = np.random.default_rng(82)
    many = np.stack([1000.0 + rng.integers(0, 8 * 100, 300) / 8.0, 2000.0 - rng.integers(0, 8 * 100, 300) / 8.0, rng.integers(4, 13, 300) / 8.0], axis=1)
    five = np.array([[1020.0, 1980.0, 6.5], [1050.25, 1950.5, 3.0], [1000.0, 2000.0, 4.0], [1099.5, 1900.5, 9.0], [1500.0, 1980.0, 2.0]])
    for mode in (HEIGHT, NDVI):
        b = full_bounds(t, rows, cols)
        out.append(_case("one_crown", raster, t, b, five[:1], mode))
        out.append(_case("300_crowns", raster, t, b, many, mode))
        out.append(_case("duplicates", raster, t, b, five[[0, 1, 0, 2, 3, 1, 4, 0, 4, 3, 2, 1]], mode, groups=[[0, 2, 7], [1, 5, 11], [3, 10], [4, 9], [6, 8]]))
    return out


FAMILIES = {"f32_rounding": _f32_rounding, "nan_pixels": _nan_pixels, "ties": _ties, "extremes": _extremes, "boundary": _boundary,
            "clipping": _clipping, "orientation": _orientation, "windows": _windows, "scale_and_grid": _scale_and_grid}
MAX_CROWNS = 64                                   # per case; scale_and_grid's 300-crown case is the one exception


@functools.lru_cache(maxsize=None)
def cases(family):
    out = tuple(FAMILIES[family]())
    assert all(c.circles.shape[0] <= MAX_CROWNS or c.name.startswith("300_crowns") for c in out)
    return out


def family_modes():
    """Every (family, mode) pair that has cases, in a fixed order."""
    return [(fam, mode) for fam in FAMILIES for mode in (HEIGHT, NDVI) if any(c.mode == mode for c in cases(fam))]


@functools.lru_cache(maxsize=None)
def expected(family, i):
    """oracle.postprocess_ref on case ``i`` of the family → float32 [n, 3] (height mode) or [n, 4] (NDVI mode), read-only."""
    case = cases(family)[i]
    px, py = vertices(case.circles)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if case.mode == HEIGHT:
            assert case.radius_scale == 1.0                # get_height_within_polygon has no radius scale
            h, xy = O.heights_within(px, py, case.raster, case.transform, case.bounds)
            return _frozen(np.column_stack([h, xy]).astype(np.float32))
        return _frozen(np.stack(O.ndvi_within(px, py, case.raster, case.transform, case.bounds, case.radius_scale), axis=1))
