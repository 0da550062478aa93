"""Crafted box-head outputs for the detection-selection stage (treedetection_amd/csrc/roi.hip: det_decode_kernel,
det_finalize_kernel; rpn.hip: sort_boxes_kernel, nms_mask_kernel, nms_scan_kernel) and crafted selections for the mask
tail (mask_predict_kernel, mask_scatter_kernel, paste_plan_kernel, paste_fill_kernel), as data only.

A case is what phase 3 of td_engine_forward_phase reads: ``proposals`` [B, P, 4], ``proposal_count`` [B] and ``box_pred``
[B * P, 6] (two logits, foreground first, then four deltas), for a batch of three images of different valid and output
sizes on one 64 x 96 frame. Rows beyond ``proposal_count[b]`` hold poison (a whole-image proposal, logits that would
score 1.0, NaN deltas): they must not influence anything. Every live row carries a tag that says what it is there for;
``expect`` holds, per image, the premises tests/test_det_cases.py proves with the oracle alone before
tests/test_det_select_gpu.py and tests/test_mask_tail_gpu.py feed the case to the engine.

``softmax64`` / ``score_tol`` are the float64 reference of the foreground score and the DERIVED bound on the engine's
float32 score (det_decode_kernel: m = max(l0, l1); e_i = expf(l_i - m); score = e0 / (e0 + e1)), with u = 2^-24:
  * l_i - m is one rounded subtraction: the argument is off by <= |d| u, d = l0 - l1, which moves exp by a factor 1 +- |d| u;
  * expf is within EXPF_ULP ulp = EXPF_ULP * 2u relative (1 ulp: the bound the HIP math API documentation states for
    expf; it is not shipped with the toolchain, so the figure is an assumption written down here);
  * one add and one divide, u each; both exponentials enter the quotient.
  => |score - score64| <= (2 (2 EXPF_ULP u + |d| u) + 2u) score64, plus 2 EXPF_ULP 2^-149 for an exponential that lands
     in the subnormals (beyond |d| = 110 that term alone: the small exponential is 0 or the least subnormal). An infinite
     |d| (one logit -inf) leaves exp(-inf) = 0 and exp(0) = 1, both exact: bound 0; so does d = 0 (1 / (1 + 1)).
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

F32 = np.float32
D = 100                         # detections_per_image
NMS_THR = 0.5
SIZE = (64, 96)                 # the padded frame: the smallest the engine accepts is 64 x 64
HW_VALID = [(64, 96), (50, 60), (61, 70)]
HW_OUT = [(96, 144), (30, 33), (77, 91)]      # x 1.5 (up), x 0.6 / 0.55 (down), x 1.26 / 1.3; none a multiple of 32 but 96
ENGINES = {"default": dict(), "thresh05": dict(score_thresh=0.5), "p130": dict(post_nms_topk=130)}
ENGINE_P = {"default": 1000, "thresh05": 1000, "p130": 130}
ENGINE_THRESH = {"default": 0.3, "thresh05": 0.5, "p130": 0.3}
U = 2.0 ** -24
EXPF_ULP = 1.0
TOL_BOX = 1e-3                  # what the project grants expf in a box decode (tests/test_rpn_select_gpu.py)
T03 = float(np.log(0.3 / 0.7))  # the logit difference that scores 0.3


def softmax64(l0, l1):
    """Foreground probability of float32 logits in float64 (NaN where the float32 softmax has NaN)."""
    l0, l1 = np.asarray(l0, np.float64), np.asarray(l1, np.float64)
    with np.errstate(all="ignore"):
        m = np.maximum(l0, l1)
        e0, e1 = np.exp(l0 - m), np.exp(l1 - m)
        return e0 / (e0 + e1)


def score_tol(l0, l1):
    """The derived bound of the module docstring, per row (NaN where the score is NaN)."""
    l0, l1 = np.asarray(l0, np.float64), np.asarray(l1, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(l0 - l1)
        s = softmax64(l0, l1)
        tol = (2.0 * (2.0 * EXPF_ULP * U + d * U) + 2.0 * U) * s + 2.0 * EXPF_ULP * 2.0 ** -149
    tol = np.where(d > 110.0, 2.0 * EXPF_ULP * 2.0 ** -149, tol)     # exp(-110) < 2^-149 / 2: the small exponential is 0 or the
    return np.where((np.isinf(d) & np.isfinite(s)) | (d == 0), 0.0, tol)   # least subnormal whatever the argument's rounding


def step(v, k):
    """float32 v moved k ulps (k < 0: down)."""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def cells(hw, ch, cw):
    """Top-left corners (x, y) of the ch x cw cells that fit the valid image, row-major."""
    h, w = hw
    return [(float(x * cw), float(y * ch)) for y in range(int(h // ch)) for x in range(int(w // cw))]


class Img:
    """Rows of one image in the making."""

    def __init__(self, hw):
        self.hw, self.box, self.pred, self.tag, self.near = hw, [], [], [], []
        self.expect: Dict[str, object] = {}

    def add(self, box, l0, l1, d=(0.0, 0.0, 0.0, 0.0), tag="", near=False):
        self.box.append([F32(v) for v in box])
        self.pred.append([F32(l0), F32(l1)] + [F32(v) for v in d])
        self.tag.append(tag)
        self.near.append(bool(near))
        return len(self.tag) - 1


def _inset(c, ch, cw, m=0.25):
    return (c[0] + m, c[1] + m, c[0] + cw - m, c[1] + ch - m)


# ---- threshold ---------------------------------------------------------------------------------------------------------
def _threshold_rows(im: Img, rng, deltas: bool, thr_logit: float, on_rows: bool):
    """Rows on, a few ulps beside, and far from the score threshold; thr_logit: l0 - l1 that scores the threshold."""
    cs = iter(cells(im.hw, 4, 4))
    rows = []
    if on_rows:                                     # l0 == l1: both exponentials are exp(0) = 1, score exactly 0.5
        for v in (0.0, 1.5, -3.0, 1e30, -1e30, 3e38, 1e-45):
            rows.append((v, v, "on", True))
        for a, b in ((1e-45, 0.0), (0.0, 1e-45), (1e-40, 0.0), (0.0, -1e-40)):    # exp(+-tiny) rounds to 1: 0.5 again
            rows.append((a, b, "on", True))
        for base, crafted in ((1.0, True), (-2.5, True), (40.0, False), (-300.0, False)):
            for k in (1, 2, 3, 4, -1, -2, -3, -4):  # a few ulps of logit above and below
                rows.append((step(base, k), base, "step", crafted))
        n_on = 11
    else:
        for l1 in (0.0, 2.0, -7.25):
            t = F32(F32(l1) + F32(thr_logit))
            for k in (1, 2, 3, 6, -1, -2, -3, -6):
                rows.append((step(t, k), l1, "step", True))
            for k in (400, -400):
                rows.append((step(t, k), l1, "step-far", False))
        n_on = 0
    for off in (3e-5, -3e-5, 1e-2, -1e-2, 0.1, -0.1, 1.0, -1.0, 5.0, -5.0, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0):
        rows.append((F32(thr_logit + off), 0.0, "above" if off > 0 else "below", False))
    order = rng.permutation(len(rows))
    for j in order:
        l0, l1, tag, near = rows[j]
        d = rng.normal(0.0, 0.3, 4) if deltas else (0.0, 0.0, 0.0, 0.0)
        im.add(_inset(next(cs), 4, 4), l0, l1, d, tag, near)
    im.expect.update(both_sides=True, **({"on": n_on} if n_on else {}))


def case_threshold(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _threshold_rows(ims[0], rng, False, 0.0, True)
    _threshold_rows(ims[1], rng, True, 0.0, True)
    cs = cells(ims[2].hw, 8, 8)
    for j, (l0, l1, tag, near) in enumerate([(2.0, 2.0, "on", True), (0.5, 0.0, "above", False), (-1.0, -1.0, "on", True),
                                             (0.0, 0.5, "below", False), (7.0, 7.0, "on", True), (3.0, 1.0, "above", False),
                                             (-4.0, 0.0, "below", False)]):
        ims[2].add(_inset(cs[j], 8, 8), l0, l1, tag=tag, near=near)
    ims[2].expect.update(on=3, both_sides=True)
    return ims


def case_threshold03(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _threshold_rows(ims[0], rng, False, T03, False)
    _threshold_rows(ims[1], rng, True, T03, False)
    _threshold_rows(ims[2], rng, False, T03, False)
    return ims


# ---- non-finite inputs, the scale clamp, overflow -------------------------------------------------------------------------
def _nonfinite_rows(im: Img, rng, deltas: bool):
    cs = iter(cells(im.hw, 6, 6))
    base = lambda: (rng.normal(0.0, 0.3, 4) if deltas else np.zeros(4))
    rows = []
    for col in range(6):
        for val in (np.nan, np.inf, -np.inf):
            r = np.concatenate([[2.0, 0.0], base()])
            r[col] = val
            rows.append((r, f"col{col}={val}"))
    rows.append((np.concatenate([[-np.inf, -np.inf], base()]), "both-logits--inf"))
    rows.append((np.concatenate([[np.inf, np.inf], base()]), "both-logits-+inf"))
    for dw, dh, tag in ((100.0, 100.0, "clamp"), (1e30, 0.0, "clamp"), (0.0, 3e38, "clamp"), (21.0, 20.7, "clamp")):
        r = np.concatenate([[2.0, 0.0], base()])
        r[4], r[5] = dw, dh
        rows.append((r, tag))
    r = np.concatenate([[2.0, 0.0], base()])               # a clamped scale that stays inside the image: a 0.5 x 0.4 px proposal
    r[4], r[5] = 100.0, 60.0                               # grows 62.5-fold to 31 x 25 px, so the box shows log(1000 / 16) itself
    rows.append((r, "clamp-small"))
    for col, val in ((2, 3e38), (3, -3e38), (2, -2e38)):
        r = np.concatenate([[2.0, 0.0], base()])
        r[col] = val
        rows.append((r, "overflow"))
    for l0, l1 in ((0.0, -np.inf), (100.0, 0.0), (200.0, 0.0), (3e38, -3e38)):
        rows.append((np.concatenate([[l0, l1], base()]), "score-1"))
    for _ in range(10):
        rows.append((np.concatenate([[rng.normal(1.5, 1.0), 0.0], base()]), "plain"))
    for j in rng.permutation(len(rows)):
        r, tag = rows[j]
        c = next(cs)                                  # (an overflow row gets the whole image as its proposal: dx / 10 * width = inf)
        box = {"overflow": (0.0, 0.0, im.hw[1], im.hw[0]), "clamp-small": (29.75, 29.8, 30.25, 30.2)}.get(tag, _inset(c, 6, 6, 0.5))
        im.add(box, r[0], r[1], r[2:], tag)
    im.expect.update(nonfinite=True)


def case_nonfinite(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _nonfinite_rows(ims[0], rng, False)
    _nonfinite_rows(ims[1], rng, True)
    _nonfinite_rows(ims[2], rng, True)
    return ims


# ---- ties ----------------------------------------------------------------------------------------------------------------
def case_ties(rng):
    ims = [Img(hw) for hw in HW_VALID]
    # image 0: 8 clusters of 50 heavily overlapping boxes, rows interleaved over the clusters, one score: rows 0..7 survive
    org = [(2.0 + 22.0 * (c % 4), 2.0 + 30.0 * (c // 4)) for c in range(8)]
    for i in range(400):
        ox, oy = org[i % 8]
        jx, jy = rng.uniform(0.0, 0.3, 2)
        ims[0].add((ox + jx, oy + jy, ox + jx + 14.0, oy + jy + 20.0), 0.25, 0.25, tag="tie")
    ims[0].expect.update(kept_rows=list(range(8)))
    # image 1: 1000 rows of one score, row i and row i + 500 share a box: rows 0..499 survive, the first 100 are kept
    cs = cells(ims[1].hw, 2, 2)
    for i in range(1000):
        ims[1].add(_inset(cs[i % 500], 2, 2), -1.0, -1.0, tag="tie")
    ims[1].expect.update(kept_rows=list(range(100)), survivors=500)
    # image 2: two scores, 1.0 and 0.5, alternating by index; duplicates 150 rows apart
    cs = cells(ims[2].hw, 3, 3)
    for i in range(300):
        one = i % 3 == 0
        ims[2].add(_inset(cs[i % 150], 3, 3), 0.0, -np.inf if one else 0.0, tag="tie-1.0" if one else "tie-0.5")
    ones = [i for i in range(150) if i % 3 == 0]
    ims[2].expect.update(kept_rows=ones + [i for i in range(150) if i % 3][: D - len(ones)], survivors=150)
    return ims


# ---- suppression chains over 64-box chunks ----------------------------------------------------------------------------------
def _chain_image(im: Img, rng, n_rows: int, n_pass: int, chains, cell=2):
    """n_rows rows, n_pass of them above the threshold with ONE score (0.5: sorted by index), every row a box of its own
    cell; chains: tuples of sorted positions (A, B[, C]): B overlaps A and C (IoU 0.54), C overlaps A by 0.25 only, so A
    suppresses B and C survives although B would have suppressed it."""
    passing = np.sort(rng.choice(n_rows, size=n_pass, replace=False))
    pos_of = {int(r): p for p, r in enumerate(passing)}
    cs = cells(im.hw, cell, cell)
    assert len(cs) >= n_rows, (len(cs), n_rows)
    member = {}
    for ch in chains:
        for j, p in enumerate(ch):
            member[p] = (ch[0], j)
    s = cell / 2.0
    for r in range(n_rows):
        p = pos_of.get(r)
        v = F32(rng.normal(0.0, 2.0))
        l0, l1 = (v, v) if p is not None else (F32(v - 3.0), v)
        if p is not None and p in member:
            a_pos, j = member[p]
            cx, cy = cs[int(passing[a_pos])]
            box = (cx + (0.1 + 0.3 * j) * s, cy + 0.1 * s, cx + (1.1 + 0.3 * j) * s, cy + 1.9 * s)
            im.add(box, l0, l1, tag="ABC"[j])
        else:
            im.add(_inset(cs[r], cell, cell, 0.1 * s), l0, l1, tag="pass" if p is not None else "below")
    im.expect.update(passing=n_pass, chains=[tuple(int(passing[p]) for p in ch) for ch in chains],
                     chain_pos=[tuple(ch) for ch in chains])


def case_chains_a(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _chain_image(ims[0], rng, 1000, 1000, [(5, 70, 140), (100, 500, 999), (63, 64, 128), (970, 980, 990)])
    _chain_image(ims[1], rng, 200, 63, [(0, 30, 62)])
    _chain_image(ims[2], rng, 200, 64, [(0, 31, 63)])
    return ims


def case_chains_b(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _chain_image(ims[0], rng, 200, 65, [(10, 64), (1, 20, 63)])
    _chain_image(ims[1], rng, 50, 1, [])
    _chain_image(ims[2], rng, 1000, 1000, [(0, 64, 960), (127, 128, 129), (959, 960 + 5, 999)])
    return ims


def case_p130(rng):
    """post_nms_topk = 130: three 64-bit words per row of the bit matrix, the last one 2 boxes wide."""
    ims = [Img(hw) for hw in HW_VALID]
    _chain_image(ims[0], rng, 130, 130, [(5, 70, 129), (63, 64, 128)], cell=4)
    _chain_image(ims[1], rng, 129, 129, [(0, 64, 128)], cell=4)
    _chain_image(ims[2], rng, 130, 65, [(3, 64)], cell=4)
    return ims


# ---- more than D survivors, empties among the first D -----------------------------------------------------------------------
def border_ulp_box(w: int):
    """A proposal (x1, x2) that, with zero deltas, decodes to [w - 1 ulp, beyond w] and so clips to a box ONE float32 ulp
    wide at the right border of a valid image w px wide: not empty for the NMS, a candidate for becoming empty in the
    output scaling. (A decode is symmetric about its centre, so away from a clipping bound it cannot yield an odd number
    of ulps.) Found by search with the oracle's own decode."""
    from oracle import ops_ref as R
    below = np.nextafter(F32(w), F32(0))
    for c in np.arange(w + 1.0, w + 14.0, 0.125):
        for a in (below, np.nextafter(below, F32(0)), F32(w)):
            b = R.apply_deltas(np.zeros((1, 4), F32), np.array([[a, 1.0, c, 3.0]], F32), (10.0, 10.0, 5.0, 5.0))
            if b[0, 0] == below and b[0, 2] > w:
                return F32(a), F32(c)
    raise AssertionError("no such proposal found")


def _over_d_image(im: Img, b: int, n_rows: int, clip_empty, ulp_merge):
    h, w = im.hw
    cs = cells(im.hw, 4, 4)
    for r in range(n_rows):
        cx, cy = cs[r]
        if r in clip_empty:                                  # wholly right of / below the valid border: clipped to zero extent
            box = (w + 1.0, cy + 0.5, w + 3.0, cy + 3.5) if clip_empty.index(r) % 2 == 0 else (cx + 0.5, h + 2.0, cx + 3.5, h + 5.0)
            tag = "clip-empty"
        elif r in ulp_merge:                                 # one ulp wide after the clip; the edges merge after * sx
            a, c = border_ulp_box(w)
            box, tag = (a, cy + 0.5, c, cy + 3.5), "ulp-merge"
        else:
            box, tag = _inset(cs[r], 4, 4, 0.5), "pass"
        im.add(box, 1.25, 1.25, tag=tag)
    empties = [r for r in range(D) if r in clip_empty or r in ulp_merge]
    im.expect.update(survivors_gt_D=True, empties_in_first_D=len(empties), count=D - len(empties))


def case_over_d(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _over_d_image(ims[0], 0, 150, [3, 50, 99, 120], [])
    _over_d_image(ims[1], 1, 150, [0, 99], [10, 64])
    _over_d_image(ims[2], 2, 150, [130], [])
    return ims


# ---- empty images between live ones ------------------------------------------------------------------------------------------
def _live(im: Img, rng, n=20):
    cs = cells(im.hw, 8, 8)
    for j in range(n):
        im.add(_inset(cs[j], 8, 8), rng.normal(0.5, 1.0), 0.0, tag="plain")
    im.expect.update(live=True)


def _all_below(im: Img, rng, n=30):
    cs = cells(im.hw, 8, 8)
    for j in range(n):
        im.add(_inset(cs[j], 8, 8), rng.uniform(-6.0, -2.0), 0.0, tag="below")
    im.expect.update(count=0)


def case_empty_a(rng):
    ims = [Img(hw) for hw in HW_VALID]
    _live(ims[0], rng)
    ims[1].expect.update(count=0, no_proposals=True)
    _all_below(ims[2], rng)
    return ims


def case_empty_b(rng):
    ims = [Img(hw) for hw in HW_VALID]
    ims[0].expect.update(count=0, no_proposals=True)
    _all_below(ims[1], rng)
    _live(ims[2], rng)
    return ims


# ---- selections for the mask tail: disjoint boxes, one score, zero deltas -------------------------------------------------------
def _special_boxes(im: Img, boxes):
    for bx in boxes:
        im.add(bx, 0.5, 0.5, tag="mask")


def case_mask_7_0_100(rng):
    ims = [Img(hw) for hw in HW_VALID]
    # image 0 (x 1.5): the whole image (touches all four borders, region 144 px wide: 4.5 words), a box under one pixel,
    # one box on each border, one 38 px wide
    _special_boxes(ims[0], [(0, 0, 96, 64), (10.2, 10.2, 10.5, 10.6), (0, 20, 8, 30), (88, 20, 96, 30), (40, 0, 50, 6),
                            (40, 58, 50, 64), (20, 36, 45.3, 50)])
    ims[0].expect.update(count=7)
    ims[1].expect.update(count=0, no_proposals=True)
    for j in range(100):
        x, y = 7.0 * (j % 10), 6.1 * (j // 10)
        ims[2].add((x + 0.5, y + 0.5, x + 6.0, y + 5.5), 0.5, 0.5, tag="mask")
    ims[2].expect.update(count=100)
    return ims


def case_mask_0_3_0(rng):
    ims = [Img(hw) for hw in HW_VALID]
    ims[0].expect.update(count=0, no_proposals=True)
    _special_boxes(ims[1], [(0, 0, 60, 50), (10, 10, 11, 11.5), (20, 20, 55, 45)])
    ims[1].expect.update(count=3)
    _all_below(ims[2], rng, 12)
    return ims


SPECS = {
    "threshold": ("thresh05", case_threshold),
    "threshold03": ("default", case_threshold03),
    "nonfinite": ("default", case_nonfinite),
    "ties": ("default", case_ties),
    "chains-a": ("default", case_chains_a),
    "chains-b": ("default", case_chains_b),
    "over_D": ("default", case_over_d),
    "empty-a": ("default", case_empty_a),
    "empty-b": ("default", case_empty_b),
    "p130": ("p130", case_p130),
}
CASE_NAMES = list(SPECS)
MASK_SPECS = {"mask-7-0-100": ("default", case_mask_7_0_100), "mask-0-3-0": ("default", case_mask_0_3_0)}
MASK_CASE_NAMES = list(MASK_SPECS)


def make_case(name: str) -> dict:
    """→ dict(name, engine, P, thresh, hw_valid, hw_out, props [B, P, 4], count [B] int32, box_pred [B * P, 6], tags [B][n],
    near [B] bool [n] (rows crafted to sit within the score tolerance of the threshold), expect [B]). Deterministic."""
    engine, fn = {**SPECS, **MASK_SPECS}[name]
    P = ENGINE_P[engine]
    rng = np.random.default_rng(list({**SPECS, **MASK_SPECS}).index(name) + 4100)
    ims: List[Img] = fn(rng)
    B = len(ims)
    props = np.empty((B, P, 4), dtype=F32)
    pred = np.empty((B, P, 6), dtype=F32)
    count = np.zeros((B,), dtype=np.int32)
    for b, im in enumerate(ims):
        n = len(im.tag)
        assert n <= P, (name, b, n)
        count[b] = n
        props[b] = (0.0, 0.0, im.hw[1], im.hw[0])            # poison beyond the count: a proposal that covers the image,
        pred[b, :, 0], pred[b, :, 1] = 1e30, -1e30           # a score of 1.0,
        pred[b, :, 2:] = np.nan                              # NaN deltas
        if n:
            props[b, :n] = np.asarray(im.box, dtype=F32)
            pred[b, :n] = np.asarray(im.pred, dtype=F32)
    return dict(name=name, engine=engine, P=P, thresh=ENGINE_THRESH[engine], hw_valid=list(HW_VALID), hw_out=list(HW_OUT),
                props=props, count=count, box_pred=np.ascontiguousarray(pred.reshape(B * P, 6)),
                tags=[list(im.tag) for im in ims], near=[np.asarray(im.near, dtype=bool) for im in ims],
                expect=[dict(im.expect) for im in ims])


def oracle_image(case: dict, b: int) -> dict:
    """The oracle on image b of a case (oracle/maskrcnn_ref.py, oracle/ops_ref.py only), in terms of the case's rows:
    decoded [n, 4] float32 apply_deltas (non-finite rows included), finite [n], boxes [n, 4] clipped, scores [n] float32
    softmax, sel [n] bool (finite and above the threshold), order: selected rows by (score descending, index), nms_rows:
    the rows NMS keeps, in order, before the cut to D; kept_rows: its first D; final boxes / scores / rows after
    detector_postprocess (paste=False)."""
    from oracle import ops_ref as R
    from oracle.maskrcnn_ref import Cfg, MaskRCNNOracle
    n = int(case["count"][b])
    P = case["P"]
    cfg = Cfg()
    cfg.score_thresh = case["thresh"]
    orc = MaskRCNNOracle({}, cfg)
    pred = case["box_pred"].reshape(-1, P, 6)[b, :n]
    props = case["props"][b, :n]
    hw = case["hw_valid"][b]
    with np.errstate(all="ignore"):
        kb, ks, taps = orc.detections(pred[:, :2], pred[:, 2:], props, hw)
        decoded = R.apply_deltas(pred[:, 2:], props, cfg.box_weights) if n else np.zeros((0, 4), F32)
        import torch
        probs = torch.softmax(torch.from_numpy(np.ascontiguousarray(pred[:, :2])), dim=-1).numpy() if n else np.zeros((0, 2), F32)
        finite = np.isfinite(decoded).all(axis=1) & np.isfinite(probs).all(axis=1)
        rows_valid = np.nonzero(finite)[0]
        assert len(rows_valid) == len(taps["all_scores"])
        sel_rows = rows_valid[taps["sel"]]
        sel = np.zeros(n, dtype=bool)
        sel[sel_rows] = True
        nms_rows = sel_rows[R.nms(taps["all_boxes"][taps["sel"]], taps["all_scores"][taps["sel"]], cfg.nms_thresh)]
        kept_rows = sel_rows[taps["keep"]]
        assert np.array_equal(kept_rows, nms_rows[:D])
        fb, fs, fr, _ = orc.postprocess(kb, ks, kept_rows, hw, case["hw_out"][b], paste=False)
    return dict(decoded=decoded, finite=finite, boxes=R.clip_boxes(decoded, hw[0], hw[1]) if n else decoded,
                scores=probs[:, 0] if n else np.zeros((0,), F32), sel=sel, nms_rows=nms_rows, kept_rows=kept_rows,
                net_boxes=kb, final_boxes=fb, final_scores=fs, final_rows=fr)


def excluded_rows(case: dict, b: int) -> np.ndarray:
    """Rows of image b whose float64 score lies within the derived tolerance of the threshold: the only rows the
    oracle-selection comparison may leave out."""
    n = int(case["count"][b])
    pred = case["box_pred"].reshape(-1, case["P"], 6)[b, :n]
    s = softmax64(pred[:, 0], pred[:, 1])
    with np.errstate(all="ignore"):
        return np.isfinite(s) & (np.abs(s - float(F32(case["thresh"]))) <= score_tol(pred[:, 0], pred[:, 1]))
