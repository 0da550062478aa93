"""The numpy oracle of the treetop rule (include/treedet.h, td_treetops) and the cases the CPU and GPU tests share. The oracle is
written from the rule, not from the library: the Gaussian table as scipy builds it, two 1-D passes in float64 in correlate1d's order
for a symmetric kernel with scipy's ``reflect`` indices, each rounded to float32 once, and the window maximum with ``np.fmax`` over
the in-range pixels (the raster padded with NaN, which fmax passes over)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "treetops")

SHAPES = [(1, 1), (1, 9), (3, 2), (2, 7), (17, 5), (5, 300), (64, 64), (65, 129), (70, 131)]      # the last three cross the tile edges
SIGMAS = (0.0, 0.5, 1.0, 2.0)           # radius 0, 2, 4, 8
WINDOWS = (1, 3, 7, 15)                 # sigma 2 with window 15 takes the kernel's 32 x 32 tile
FLOOR = 3.0


def weights(sigma, truncate=4.0):
    r = int(truncate * sigma + 0.5)
    if r == 0:
        return np.ones(1)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def reflect_idx(i, n):
    """scipy 'reflect': d c b a | a b c d | d c b a"""
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i >= n, p - 1 - i, i)


def pass1d(a32, axis, w):
    r = (w.size - 1) // 2
    a = np.moveaxis(a32, axis, 0).astype(np.float64)
    idx = np.arange(a.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        t = a[idx] * w[r]
        for ii in range(-r, 0):
            t = t + (a[reflect_idx(idx + ii, a.shape[0])] + a[reflect_idx(idx - ii, a.shape[0])]) * w[r + ii]
        return np.moveaxis(t.astype(np.float32), 0, axis)


def smooth(a32, w):
    return pass1d(pass1d(a32, 0, w), 1, w)


def window_max(s, k):
    h = k // 2
    rows, cols = s.shape
    padded = np.full((rows + 2 * h, cols + 2 * h), np.nan, s.dtype)
    padded[h:h + rows, h:h + cols] = s
    out = np.full(s.shape, np.nan, s.dtype)
    for dr in range(k):
        for dc in range(k):
            out = np.fmax(out, padded[dr:dr + rows, dc:dc + cols])
    return out


def oracle(a32, w, k, floor):
    """→ (marks uint8, smoothed float32)"""
    s = smooth(np.ascontiguousarray(a32, dtype=np.float32), np.asarray(w, np.float64))
    with np.errstate(invalid="ignore"):
        marks = (s > np.float32(floor)) & (s >= window_max(s, k))
    return marks.astype(np.uint8), s


def same_floats(a, b):
    """Bit for bit, a NaN being a NaN (include/treedet.h: its sign and payload are not part of the rule)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all()) and bool((a.view(np.uint32)[~nan] == b.view(np.uint32)[~nan]).all())


def canopy(shape, seed, plateaus):
    """Random heights in [0, 30) m with 30 % zeros; ``plateaus``: quantised to 4 m, so that neighbours tie."""
    rng = np.random.default_rng(seed)
    a = (rng.random(shape) * 30).astype(np.float32)
    a[rng.random(shape) < 0.3] = 0.0
    return (np.round(a / 4) * 4).astype(np.float32) if plateaus else a


def random_cases(shape):
    """Every sigma x window x value type on one shape → (name, raster, weights, window, floor)"""
    out = []
    for si, sigma in enumerate(SIGMAS):
        for wi, k in enumerate(WINDOWS):
            for plateaus in (False, True):
                seed = 1000 * SHAPES.index(shape) + 100 * si + 10 * wi + int(plateaus)
                out.append((f"{shape[0]}x{shape[1]}-s{sigma}-k{k}-{'plateau' if plateaus else 'random'}", canopy(shape, seed, plateaus),
                            weights(sigma), k, FLOOR))
    return out


def spike(shape, at, value=10.0):
    a = np.zeros(shape, np.float32)
    for r, c in at:
        a[r, c] = value
    return a


def crafted_cases():
    """(name, raster, weights, window, floor, expected) — expected: the (row, col) list the marks must equal, or None (oracle only)"""
    shape = (70, 131)
    out = []
    for at in [(0, 0), (69, 130), (63, 63), (63, 64), (64, 64)]:          # corners of the raster and of the 64 x 64 tiles
        for sigma in (0.0, 0.5):
            out.append((f"spike-{at[0]}-{at[1]}-s{sigma}", spike(shape, [at]), weights(sigma), 7, FLOOR, [at]))
    for sigma in (0.0, 0.5):
        # 3 columns apart: each lies in the other's 7-wide window and equals it — both are treetops; 4 apart: neither sees the other
        out.append((f"twins-3-apart-s{sigma}", spike(shape, [(40, 62), (40, 65)]), weights(sigma), 7, FLOOR, [(40, 62), (40, 65)]))
        out.append((f"twins-4-apart-s{sigma}", spike(shape, [(40, 61), (40, 65)]), weights(sigma), 7, FLOOR, [(40, 61), (40, 65)]))
    f32 = np.float32(FLOOR)
    out.append(("spike-at-the-floor", spike(shape, [(5, 5)], f32), weights(0.0), 7, FLOOR, []))
    out.append(("spike-one-ulp-above", spike(shape, [(5, 5)], np.nextafter(f32, np.float32(np.inf))), weights(0.0), 7, FLOOR, [(5, 5)]))
    for sigma in SIGMAS:
        for k in (3, 7):
            rng = np.random.default_rng(77 + k)
            a = canopy(shape, 500 + k, plateaus=True)
            for value in (np.nan, np.inf, -np.inf):
                a[rng.random(shape) < 0.01] = value
            a[0, 0], a[69, 130], a[63, 64] = np.nan, np.inf, -np.inf
            out.append((f"nonfinite-s{sigma}-k{k}", a, weights(sigma), k, FLOOR, None))
    out.append(("all-nan", np.full((9, 70), np.nan, np.float32), weights(0.5), 7, FLOOR, []))
    out.append(("floor-minus-inf", canopy((17, 5), 9, True), weights(0.5), 3, -np.inf, None))
    return out


def golden_cases():
    """The recorded scipy results (tests/golden/treetops/*.npz, written by tests/golden/make_treetops_golden.py with scipy 1.15.3):
    → (name, raster, sigma, window, floor, scipy's gaussian_filter, scipy's argwhere rows / cols)"""
    out = []
    for name in sorted(os.listdir(GOLDEN)):
        if name.endswith(".npz"):
            z = np.load(os.path.join(GOLDEN, name))
            out.append((name[:-4], z["raster"], float(z["sigma"]), int(z["window"]), float(z["floor"]), z["smoothed"], z["tops"]))
    return out


# ---- a crown-stage scene with known treetops (tests/test_postprocessing_treetops*.py) --------------------------------------------
HT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318120.0)             # the nDSM: 60 x 60 pixels of 1 m
IT = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)             # the image: 300 x 300 pixels of 0.2 m
GROUND = 2.5                                                 # under the default floor of 3 m, over the scene's height_threshold of 2


def _hexagon(cx, cy, r):
    return [(cx + r * np.cos(a), cy + r * np.sin(a)) for a in np.deg2rad([10, 70, 130, 190, 250, 310])]


# (outline in metres east and SOUTH of the rasters' corner, score, treetops inside as constructed)
SCENE_CROWNS = [(_hexagon(14.0, 14.0, 7.0), 0.9, 2),                                        # A: its own top and the one it shares with B
                (_hexagon(22.3, 17.1, 6.0), 0.6, 1),                                        # B: reaches into A, the lower score: the shared top only
                ([(34.3, 30.2), (46.7, 31.1), (45.9, 40.6), (35.2, 39.8)], 0.7, 0),         # C: none
                ([(41.2, 35.3), (53.6, 36.4), (52.8, 47.9), (42.1, 46.6)], 0.7, 1),         # D: reaches into C, the same score; one top outside C
                ([(10.2, 38.4), (23.7, 41.3), (14.6, 53.2)], 0.5, 2)]                       # E: two tops
# (row, col, height of the spike, 1-based crown that owns the top: the highest score that holds it, or 0) in row-major order
SCENE_TOPS = [(5, 50, 9.0, 0), (14, 14, 12.0, 1), (15, 19, 11.0, 1), (42, 14, 10.0, 5), (44, 50, 13.0, 4), (47, 16, 14.0, 5)]


def scene_ring(points):
    """A closed ring in map coordinates."""
    pts = list(points) + [points[0]]
    return np.array([(HT[2] + x, HT[5] - y) for x, y in pts])


def scene_height():
    a = np.full((60, 60), GROUND, np.float32)
    for r, c, v, _ in SCENE_TOPS:
        a[r, c] = v
    return a


def inside(ring, x, y):
    """Even-odd, half-open in y: is (x, y) inside the closed ring (no point of the scene lies on an edge)."""
    hit = False
    for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]):
        if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
            hit = not hit
    return hit


def scene_expectation(rings, scores, tops_rc):
    """(treetops per ring, 1-based owner per top) by the even-odd test over the pixel centres, the highest score first and among
    equal scores the lower index."""
    per_ring, owner = [0] * len(rings), []
    for r, c in tops_rc:
        x, y = HT[2] + (c + 0.5), HT[5] - (r + 0.5)
        holds = [k for k, ring in enumerate(rings) if inside(np.asarray(ring), x, y)]
        for k in holds:
            per_ring[k] += 1
        owner.append(1 + min(holds, key=lambda k: (-scores[k], k)) if holds else 0)
    return per_ring, owner
