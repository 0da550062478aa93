"""The cases the evaluation tests share (tests/test_evaluation.py on the CPU, tests/test_evaluation_gpu.py on the device): box
sets for the two-set pair search with its numpy brute force, the dense restatement of the reference's matching loop, the grid of
squares with hand-derived scores, and the seeded blob-crown scene. Seeded; nothing here loads the library."""
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_iou_ref as R  # noqa: E402

NAN = float("nan")


# ---- box pairs ------------------------------------------------------------------------------------------------------------------
def brute_pairs(a, b):
    """The pair rule as it is written, O(n_a n_b): min(x2_i, x2_j) > max(x1_i, x1_j) and likewise y (numpy's minimum / maximum hand a
    NaN on, and a NaN fails the comparison) → int32 [k, 2], sorted lexicographically."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 4), np.asarray(b, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        x = np.minimum(a[:, None, 2], b[None, :, 2]) > np.maximum(a[:, None, 0], b[None, :, 0])
        y = np.minimum(a[:, None, 3], b[None, :, 3]) > np.maximum(a[:, None, 1], b[None, :, 1])
    return np.argwhere(x & y).astype(np.int32).reshape(-1, 2)


def jittered_boxes(rng, n, side, pitch, lo, hi):
    """n boxes on a jittered grid ``side`` wide: centres pitch apart and moved by up to a pitch, widths and heights in [lo, hi)."""
    k = np.arange(n)
    c = np.stack([pitch * (k % side), pitch * (k // side)], axis=1) + rng.uniform(-pitch, pitch, (n, 2)) + np.array([412000.0, 5318000.0])
    half = rng.uniform(lo, hi, (n, 2)) / 2
    return np.concatenate([c - half, c + half], axis=1)


def _nan_slots():
    """A box with a NaN in each coordinate slot, once on the A side and once on the B side, against boxes that would overlap it."""
    good = np.array([[0.0, 0.0, 4.0, 4.0], [1.0, 1.0, 3.0, 3.0]])
    bad = np.tile(np.array([[0.5, 0.5, 3.5, 3.5]]), (4, 1))
    bad[np.arange(4), np.arange(4)] = NAN
    return np.concatenate([bad, good]), np.concatenate([good, bad, np.full((1, 4), NAN)])


@lru_cache(maxsize=None)
def box_cases():
    """name → (boxes_a, boxes_b), float64 [n, 4]."""
    rng = np.random.default_rng(20251021)
    unit = np.array([[0.0, 0.0, 1.0, 1.0]])
    out = {
        "touching_edge": (unit, np.array([[1.0, 0.0, 2.0, 1.0], [0.0, 1.0, 1.0, 2.0], [-1.0, 0.0, 0.0, 1.0], [0.0, -1.0, 1.0, 0.0]])),
        "touching_corner": (unit, np.array([[1.0, 1.0, 2.0, 2.0], [-1.0, -1.0, 0.0, 0.0], [1.0, -1.0, 2.0, 0.0], [-1.0, 1.0, 0.0, 2.0]])),
        "a_hair_inside": (unit, np.array([[np.nextafter(1.0, 0.0), np.nextafter(1.0, 0.0), 2.0, 2.0], [np.nextafter(1.0, 0.0), 1.0, 2.0, 2.0]])),
        "identical": (np.tile(unit, (3, 1)), np.tile(unit, (2, 1))),
        "zero_width": (np.array([[0.5, 0.0, 0.5, 1.0], [0.0, 0.5, 1.0, 0.5], [0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5]]),
                       np.array([[-1.0, -1.0, 2.0, 2.0], [0.5, -1.0, 0.5, 2.0], [0.25, 0.25, 0.75, 0.75]])),
        "inverted": (np.array([[1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]]), np.array([[-1.0, -1.0, 2.0, 2.0], [2.0, 2.0, -1.0, -1.0]])),
        "infinite": (np.array([[-np.inf, -np.inf, np.inf, np.inf], [0.0, 0.0, np.inf, 1.0]]), np.array([[5.0, 0.5, 6.0, 0.75], [-3.0, -3.0, -2.0, -2.0]])),
        "nan_slots": _nan_slots(),
        "utm_far_apart": (np.array([[412000.0, 5318000.0, 412000.0 + 2.0 ** 26, 5318010.0]]),
                          np.array([[412000.0 + 2.0 ** 26 - 1e-7, 5318005.0, 412000.0 + 2.0 ** 27, 5318006.0], [412000.0 + 2.0 ** 26, 5318005.0, 412000.0 + 2.0 ** 27, 5318006.0]])),
    }
    one = jittered_boxes(rng, 1, 1, 5.0, 8.0, 9.0)
    some = jittered_boxes(rng, 5, 2, 5.0, 8.0, 9.0)
    out["0x0"] = (np.zeros((0, 4)), np.zeros((0, 4)))
    out["0x5"] = (np.zeros((0, 4)), some)
    out["5x0"] = (some, np.zeros((0, 4)))
    out["1x1"] = (one, one + 0.5)
    out["1x5"] = (one, some)
    out["5x1"] = (some, one)
    out["257x1025"] = (jittered_boxes(rng, 257, 17, 6.0, 3.0, 9.0), jittered_boxes(rng, 1025, 33, 3.0, 2.0, 7.0))      # a ragged second row block and column chunk
    out["1025x257"] = (out["257x1025"][1], out["257x1025"][0])
    out["700x900"] = (jittered_boxes(rng, 700, 27, 5.0, 2.0, 9.0), jittered_boxes(rng, 900, 30, 4.5, 2.0, 9.0))
    return out


@lru_cache(maxsize=None)
def heavy_overlap():
    """3000 x 2100 boxes of 5 - 30 units in a 250 x 250 field: a few hundred thousand pairs, rows of very different lengths."""
    rng = np.random.default_rng(77)

    def boxes(n):
        c = rng.uniform(0, 250, (n, 2)) + np.array([412000.0, 5318000.0])
        half = rng.uniform(2.5, 15.0, (n, 2))
        return np.concatenate([c - half, c + half], axis=1)

    return boxes(3000), boxes(2100)


# ---- the matching loop ----------------------------------------------------------------------------------------------------------
def dense_calculate_iou(iou, candidates, iou_threshold):
    """The loop of the reference's ``calculate_iou`` restated line by line on a dense matrix: ``iou`` float64 [m, n], ``candidates``
    bool [m, n] = what ``ann_strtree.query(pred_geom)`` returns for prediction p, as positions; ``ann.index`` is 0 .. n - 1.
    The reference's ``if not np.any(candidates): continue`` is deliberately NOT restated (the module docstring of
    treedetection_amd/evaluation.py says why); an empty candidate list leaves the loop two lines further down as it does there.
    → (tp_list, fp_list, fn_list, matched annotation per prediction or -1, mean_iou)"""
    m, n = iou.shape
    pred_matched, ann_matched, iou_scores = set(), set(), []
    match_of_pred = np.full(m, -1, np.int64)
    for p_idx in range(m):
        cand = np.flatnonzero(candidates[p_idx])
        candidate_indices = cand
        iou_values = iou[p_idx, cand]
        if len(iou_values) == 0:
            continue
        unmatched_mask = ~np.isin(candidate_indices, list(ann_matched))
        iou_values = iou_values[unmatched_mask]
        candidate_indices = candidate_indices[unmatched_mask]
        if len(iou_values) == 0:
            continue
        max_iou_idx = np.argmax(iou_values)
        max_iou = iou_values[max_iou_idx]
        if max_iou >= iou_threshold:
            pred_matched.add(p_idx)
            ann_matched.add(int(candidate_indices[max_iou_idx]))
            match_of_pred[p_idx] = candidate_indices[max_iou_idx]
            iou_scores.append(max_iou)
    mean_iou = np.mean(iou_scores) if iou_scores else 0.0
    tp_list = np.zeros(m, dtype=bool)
    fp_list = np.ones(m, dtype=bool)
    fn_list = np.ones(n, dtype=bool)
    for p_idx in pred_matched:
        tp_list[p_idx] = True
        fp_list[p_idx] = False
    for a_idx in ann_matched:
        fn_list[a_idx] = False
    return tp_list, fp_list, fn_list, match_of_pred, mean_iou


def csr_of(iou, candidates):
    """Dense [m, n] → (row_start, cols ascending within a row, iou) over the candidate entries."""
    m = iou.shape[0]
    rows, cols = np.nonzero(candidates)
    row_start = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=row_start[1:])
    return row_start, cols.astype(np.int32), np.ascontiguousarray(iou[rows, cols], dtype=np.float64)


# ---- the grid of squares --------------------------------------------------------------------------------------------------------
X0, Y0 = 412000.0, 5318000.0
SIDE = 10.0


def square(x, y, s=SIDE):
    """A closed ring, counter-clockwise."""
    return np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s], [x, y]], dtype=np.float64)


# Annotations A0 .. A4: squares of side 10, 20 apart along x. A prediction moved by dx along x from its annotation has
# IoU = (10 - dx) / (10 + dx): dx 0 → 1, 1 → 9/11 = 0.818, 2 → 8/12 = 0.667, 4 → 6/14 = 0.429, 7 → 3/17 = 0.176.
GRID_IOU_THRESHOLDS = (0.3, 0.5, 0.75)
GRID_CONFIDENCE_THRESHOLDS = (0.3, 0.5, 0.7, 0.95, 0.99)
GRID_MARGIN = 0.05          # every IoU above lies at least this far from every IoU threshold


def grid_scene():
    """(prediction rings, scores, annotation rings, expected IoU per prediction as (annotation, numerator, denominator) or None)."""
    ann = [square(X0 + 20.0 * k, Y0) for k in range(5)]
    pred = [(0, 4.0, 0.9),        # P0: A0 at IoU 0.429 — first in the file, so at t = 0.3 it takes A0 ...
            (0, 1.0, 0.8),        # P1: A0 at IoU 0.818 — ... which the later, better P1 then cannot have
            (1, 0.0, 0.6),        # P2: A1 exactly
            (2, 2.0, 0.4),        # P3: A2 at IoU 0.667
            (3, 7.0, 0.95)]       # P4: A3 at IoU 0.176: never a match
    rings = [square(X0 + 20.0 * k + dx, Y0) for k, dx, _ in pred] + [square(X0, Y0 + 100.0)]      # P5: overlaps nothing
    scores = [s for _, _, s in pred] + [0.35]
    expect = [(k, SIDE - dx, SIDE + dx) for k, dx, _ in pred] + [None]
    return rings, scores, ann, expect


# (iou threshold, confidence threshold) → (tp, fp, fn, tp_list over the selected predictions, fn_list) — derived by hand from the
# comments above. Selected: c 0.3 → P0 .. P5; 0.5 → P0 P1 P2 P4; 0.7 → P0 P1 P4; 0.95 → P4; 0.99 → nothing (no record).
T, F = True, False
GRID_EXPECTED = {
    (0.3, 0.3): (3, 3, 2, [T, F, T, T, F, F], [F, F, F, T, T]),       # P0-A0, P2-A1, P3-A2
    (0.3, 0.5): (2, 2, 3, [T, F, T, F], [F, F, T, T, T]),
    (0.3, 0.7): (1, 2, 4, [T, F, F], [F, T, T, T, T]),
    (0.3, 0.95): (0, 1, 5, [F], [T, T, T, T, T]),
    (0.5, 0.3): (3, 3, 2, [F, T, T, T, F, F], [F, F, F, T, T]),       # P0 falls short, P1-A0
    (0.5, 0.5): (2, 2, 3, [F, T, T, F], [F, F, T, T, T]),
    (0.5, 0.7): (1, 2, 4, [F, T, F], [F, T, T, T, T]),
    (0.5, 0.95): (0, 1, 5, [F], [T, T, T, T, T]),
    (0.75, 0.3): (2, 4, 3, [F, T, T, F, F, F], [F, F, T, T, T]),      # P3 falls short too
    (0.75, 0.5): (2, 2, 3, [F, T, T, F], [F, F, T, T, T]),
    (0.75, 0.7): (1, 2, 4, [F, T, F], [F, T, T, T, T]),
    (0.75, 0.95): (0, 1, 5, [F], [T, T, T, T, T]),
}
GRID_MATCHED_IOUS = {           # the matched IoUs in matching order, as fractions (numerator, denominator)
    (0.3, 0.3): [(6, 14), (10, 10), (8, 12)], (0.3, 0.5): [(6, 14), (10, 10)], (0.3, 0.7): [(6, 14)], (0.3, 0.95): [],
    (0.5, 0.3): [(9, 11), (10, 10), (8, 12)], (0.5, 0.5): [(9, 11), (10, 10)], (0.5, 0.7): [(9, 11)], (0.5, 0.95): [],
    (0.75, 0.3): [(9, 11), (10, 10)], (0.75, 0.5): [(9, 11), (10, 10)], (0.75, 0.7): [(9, 11)], (0.75, 0.95): [],
}


# ---- blob crowns ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def blob_scene(n=400, seed=11):
    """(prediction rings, scores, annotation rings): n star-shaped blob crowns of 8 - 24 vertices on a jittered grid at UTM
    coordinates (neighbours overlap), every seventh followed by a near-duplicate; the annotations are shifted and rescaled copies
    of about three quarters of them (the rest deleted) in another order, plus a few crowns nobody predicted. The last prediction
    and the last annotation are rings of 700 and 400 vertices that overlap: one pair above the area kernel's 1 024-vertex cap."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    pred, k = [], 0
    while len(pred) < n:
        c = np.array([X0 + 5.0 * (k % side), Y0 + 5.0 * (k // side)]) + rng.uniform(-1.0, 1.0, 2)
        ring = R.star(rng, int(rng.integers(8, 25)), c, 2.0, 3.6)
        pred.append(ring)
        if k % 7 == 3:
            pred.append(c + (ring - c) * rng.uniform(0.85, 0.97) + rng.uniform(-0.1, 0.1, 2))
        k += 1
    pred = pred[:n]
    ann = []
    for ring in pred:
        if rng.uniform() < 0.75:
            c = ring.mean(axis=0)
            ann.append(c + (ring - c) * rng.uniform(0.7, 1.2) + rng.uniform(-0.9, 0.9, 2))
    for _ in range(12):
        ann.append(R.star(rng, int(rng.integers(8, 25)), np.array([X0, Y0]) + rng.uniform(0, 5.0 * side, 2), 1.5, 3.0))
    ann = [ann[i] for i in rng.permutation(len(ann))]
    far = np.array([X0 - 60.0, Y0 - 60.0])
    pred.append(R.star(rng, 700, far, 8.0, 9.0))
    ann.append(R.star(rng, 400, far + 1.5, 7.0, 8.5))
    scores = [float(v) for v in np.round(rng.uniform(0.2, 1.0, len(pred)), 3)]
    close = lambda r: np.concatenate([r, r[:1]])
    return [close(r) for r in pred], scores, [close(r) for r in ann]
