"""Shared inputs of the box-pair filter tests (test_pair_filters.py, test_pair_filters_gpu.py): seeded case families for
filter_polygons_by_iou_and_area and containment. Not a test. ``make(family, n, seed)`` → a :class:`Case` of exactly ``n`` crowns: the
family's crafted crowns, in their order, spread between filler crowns of family "a" so that they straddle the kernels' tile edges.

  a  random circles at the density of tools/crown_bench.py (20 000 crowns of 1.5 - 6 m radius on 980 m x 980 m) at UTM coordinates
     (412 000 / 5 318 000): float32 has 1/32 m steps in x and 0.5 m steps in y there, so the quantisation of the boxes is live
  b  clusters of 2 - 6 near-duplicate boxes with near-equal areas (area threshold 0.25: some members connect, some do not)
  c  chains A ~ B, B ~ C with A !~ C, scores falling along the chain: B is removed by A's group and is still the best of C's
  d  clusters whose scores differ in float64 and are equal in float16 (the tie rule), some members with a float16 area of 0,
     whose mask diagonal is 0 / 0 = NaN = unset while they stay connected to the others (area threshold 3)
  e  IoU exactly at the threshold ([0,0,2,2] against [0,0,2,1] at 0.5: not ``>``) and containment exactly at it ([0,0,2,2] against
     [0,0,4,1] at 0.5: ``>=`` holds), at small power-of-two offsets so that every value is exact
  f  nested boxes: outers that contain 0, 1, 2, 3, 4, 5 others, and partial overlaps on either side of the 0.9 threshold
"""
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

FAMILIES = ("a", "b", "c", "d", "e", "f")
X0, Y0 = 412000.0, 5318000.0
DENSITY = 20000 / (980.0 * 980.0)                  # crowns per square metre (tools/crown_bench.py)


@dataclass
class Case:
    bounds: List[Tuple[float, float, float, float]]
    areas: List[float]
    scores: List[float]
    iou_threshold: float
    area_threshold: float
    containment_threshold: float


def _side(n):
    return max(40.0, float(np.sqrt(max(n, 1) / DENSITY)))


def _circles(rng, n, side):
    cx, cy, r = rng.uniform(X0 + 10, X0 + 10 + side, n), rng.uniform(Y0 + 10, Y0 + 10 + side, n), rng.uniform(1.5, 6.0, n)
    boxes = [(float(x - q), float(y - q), float(x + q), float(y + q)) for x, y, q in zip(cx, cy, r)]
    areas = [float(np.pi * q * q * u) for q, u in zip(r, rng.uniform(0.8, 1.0, n))]
    return boxes, areas, [float(s) for s in rng.uniform(0.3, 1.0, n)]


def _crafted(family, rng, budget, side):
    """Up to ``budget`` crafted crowns of one family → (boxes, areas, scores)."""
    boxes, areas, scores = [], [], []

    def add(box, area, score):
        boxes.append(tuple(float(v) for v in box))
        areas.append(float(area))
        scores.append(float(score))

    if family == "a":
        return boxes, areas, scores
    k = 0
    while len(boxes) < budget:
        cx, cy = rng.uniform(X0 + 20, X0 + 20 + side), rng.uniform(Y0 + 20, Y0 + 20 + side)
        if family == "b":
            r, area = rng.uniform(2.0, 6.0), rng.uniform(20.0, 100.0)
            for _ in range(int(rng.integers(2, 7))):
                dx, dy, dr = rng.uniform(-0.3, 0.3, 3)
                add((cx + dx - r - dr, cy + dy - r, cx + dx + r + dr, cy + dy + r), area * (1 + rng.uniform(-0.2, 0.2)), rng.uniform(0.3, 1.0))
        elif family == "c":
            w, top = 16.0, rng.uniform(0.6, 0.95)
            for m in range(int(rng.integers(3, 6))):       # each link shifted by 0.3 w: IoU 0.7 / 1.3 = 0.54 with the next, 0.25 with the one after
                add((cx + 0.3 * w * m, cy, cx + 0.3 * w * m + w, cy + w), 200.0, top - 0.05 * m)
        elif family == "d":
            r, s = rng.uniform(2.0, 6.0), float(np.float16(rng.uniform(0.4, 0.95)))
            for m in range(int(rng.integers(2, 6))):
                area = 0.0 if rng.uniform() < 0.3 else 50.0
                add((cx - r, cy - r, cx + r, cy + r + 0.01 * m), area, s + 1e-5 * rng.integers(0, 8))
        elif family == "e":
            ox, oy = 64.0 * k, 16.0 * (k % 3)              # exact in float32, groups apart from each other
            add((ox, oy, ox + 2, oy + 2), 4.0, 0.9)
            add((ox, oy, ox + 2, oy + 1), 4.0, 0.8)        # IoU 2 / 4 with the first
            add((ox + 8, oy, ox + 10, oy + 2), 4.0, 0.7)
            add((ox + 8, oy, ox + 12, oy + 1), 4.0, 0.6)   # half of it lies in the third: ratio 2 / 4
            add((ox + 16, oy, ox + 18, oy + 2), 4.0, 0.5)
            add((ox + 16, oy, ox + 18, oy + 1.25), 4.0, 0.4)   # IoU 2.5 / 4 = 0.625 with the fifth: connected
        else:                                              # f
            inner = k % 6
            add((cx, cy, cx + 24, cy + 8), 150.0, rng.uniform(0.3, 1.0))
            for m in range(inner):
                add((cx + 1 + 4 * m, cy + 1, cx + 3.5 + 4 * m, cy + 3), 6.0, rng.uniform(0.3, 1.0))
            if k % 2:
                add((cx + 22, cy + 5, cx + 22 + 2.0 / rng.choice([0.8, 0.95]), cy + 7), 5.0, rng.uniform(0.3, 1.0))   # 80 % / 95 % inside
        k += 1
    return boxes[:budget], areas[:budget], scores[:budget]


THRESHOLDS = {"a": (0.5, 3, 0.9), "b": (0.5, 0.25, 0.9), "c": (0.5, 3, 0.9), "d": (0.5, 3, 0.9), "e": (0.5, 3, 0.5), "f": (0.5, 1, 0.9)}


def make(family: str, n: int, seed: int = 0) -> Case:
    assert family in FAMILIES and n >= 0
    rng = np.random.default_rng([seed, FAMILIES.index(family), n])
    side = _side(n)
    crafted = _crafted(family, rng, n if n <= 8 else (2 * n) // 3, side)
    m = len(crafted[0])
    filler = _circles(rng, n - m, side)
    slots = np.zeros(n, bool)
    slots[np.sort(rng.choice(n, m, replace=False))] = True      # the crafted crowns keep their order
    it_c, it_f = (iter(zip(*crafted)), iter(zip(*filler)))
    rows = [next(it_c) if s else next(it_f) for s in slots]
    iou_thr, area_thr, contain_thr = THRESHOLDS[family]
    return Case([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], iou_thr, area_thr, contain_thr)


def oracle_mask(case: Case) -> np.ndarray:
    """The N x N mask of oracle.postprocess_ref.filter_by_iou_and_area (its first lines, the diagonal included)."""
    from oracle import postprocess_ref as O
    bb = np.array([[np.float32(v) for v in b] for b in case.bounds], dtype=np.float32).reshape(-1, 4)
    ar = np.array(case.areas, dtype=np.float16)
    iou = O.box_iou(bb, bb)
    with np.errstate(divide="ignore", invalid="ignore"):
        area_diff = np.abs(ar[:, None] - ar) / np.maximum(ar[:, None], ar)
    return (iou > case.iou_threshold) & (area_diff < case.area_threshold)
