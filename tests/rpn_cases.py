"""Crafted RPN head outputs for the proposal-selection stage (treedetection_amd/csrc/rpn.hip) at production map sizes, and a
numpy restatement of the rule by which rpn_topk_decode_kernel picks one of its three code paths.

``regime(logits, k)`` restates the dispatch from the comment block above the kernel — order-preserving integer key of the
float, 4096-bin histogram of the keys' top 12 bits, highest bins first, fast path when the bin that holds the k-th key and
all higher bins hold <= 4096 keys; otherwise a radix select whose compaction is unordered when every key equal to the
k-th belongs to the top-k and ordered when the tie straddles the cut. It does not call the library.

The generators return per-level ``[B, h*w*3]`` logits and ``[B, h*w*3, 4]`` deltas in the oracle's (y, x, anchor) order,
and, per image and level, the path the case intends to reach. tests/test_rpn_cases.py proves on the CPU that every case
reaches what it intends; tests/test_rpn_select_gpu.py feeds the cases to the engine.

NaN logits are deliberately absent: numpy sorts NaN last, torch sorts it first, so ``oracle/ops_ref.py`` is no reference
for them. NaN and inf DELTAS are present (the candidate is dropped after the top-k, by both sides).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

F32 = np.float32
A = 3                       # anchors per position
K = 1000                    # pre_nms_topk
POST_K = 1000               # post_nms_topk
HIST_BITS = 12
TOPK_FAST = 4096
ROUND = 1024                # keys per round of the ordered compaction (one block of 1024 threads)
SIZES = {"800x800": (800, 800), "800x1344": (800, 1344)}
HW_VALID = {"800x800": [(800, 800), (750, 620)], "800x1344": [(800, 1333), (613, 1333)]}
ONE = 0x3F800000            # bits of 1.0f; [1.0, 1.125) is one bin of the coarse histogram (2**20 floats)
BIN_FLOATS = 1 << 20


# ---- the dispatch rule ------------------------------------------------------------------------------------------------
def float_to_key(x: np.ndarray) -> np.ndarray:
    """uint32 whose unsigned order is the floats' order; -0.0 and +0.0 share one key."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def regime(logits: np.ndarray, k: int = K) -> Tuple[str, int]:
    """("fast" | "unordered" | "ordered", number of keys in the threshold bin and all higher bins)."""
    key = float_to_key(np.asarray(logits).reshape(-1))
    n = key.size
    k = min(k, n)
    assert k > 0
    hist = np.bincount(key >> np.uint32(32 - HIST_BITS), minlength=1 << HIST_BITS)
    down = np.cumsum(hist[::-1])                      # down[j]: keys in the j + 1 highest bins
    j = int(np.searchsorted(down, k, side="left"))    # first (highest) bin at which the count reaches k
    cand = int(down[j])
    if cand <= TOPK_FAST:
        return "fast", cand
    thr = np.sort(key)[n - k]                         # the k-th largest key
    need_eq = k - int((key > thr).sum())
    eq_total = int((key == thr).sum())
    return ("unordered" if eq_total == need_eq else "ordered"), cand


def level_shapes(hp: int, wp: int) -> List[Tuple[int, int]]:
    """(h, w) of p2..p6 for a padded batch of hp x wp (p6 = p5 subsampled by 2)."""
    hw = [(hp >> (l + 2), wp >> (l + 2)) for l in range(4)]
    return hw + [((hw[3][0] - 1) // 2 + 1, (hw[3][1] - 1) // 2 + 1)]


# ---- logit families: each returns (float32 [n], intended regime when n allows a general path) ----------------------------
def _one_bin_distinct(rng, n, lo=0, hi=BIN_FLOATS):
    """n distinct floats of [1.0, 1.125), in random order."""
    return (np.uint32(ONE) + rng.choice(np.arange(lo, hi, dtype=np.uint32), size=n, replace=False)).view(F32)


def spread(rng, n):
    return rng.normal(-4.0, 2.0, n).astype(F32), "fast"


def spread_eighths(rng, n):
    """Ties inside the sort and at the cut, still a few thousand candidates."""
    return (np.round(rng.normal(-6.0, 1.0, n) * 8.0) / 8.0).astype(F32), "fast"


def mixed_sign(rng, n):
    return rng.normal(0.0, 3.0, n).astype(F32), "fast"


def _tie_pairs_inside_topk(v, k=K):
    """Every 7th rank of the top-k takes the value of the rank above it (in place): ties for the sort to break by index,
    none of them near the cut, so the k-th key stays unique."""
    if v.size > k + 1:
        order = np.argsort(-v.astype(np.float64), kind="stable")
        r = np.arange(10, k - 100, 7)
        v[order[r + 1]] = v[order[r]]
    return v


def near_constant(rng, n):
    """All keys in one coarse bin, distinct but for tied pairs inside the top-k: the whole radix select, clean cut."""
    return _tie_pairs_inside_topk(_one_bin_distinct(rng, n)), "unordered"


def near_constant_512ths(rng, n):
    """The same rounded to 1/512: 64 values, the cut falls inside a tie."""
    v = _one_bin_distinct(rng, n)
    return (np.floor(v * F32(512.0)) / F32(512.0)).astype(F32), "ordered"


def negative_near_constant(rng, n):
    """Negative-only logits in one bin (inverted keys), distinct but for tied pairs inside the top-k."""
    return _tie_pairs_inside_topk((-_one_bin_distinct(rng, n)).astype(F32)), "unordered"


def all_equal(value):
    def f(rng, n):
        return np.full(n, value, dtype=F32), "ordered"
    return f


def signed_zeros_all(rng, n):
    """Every logit is a zero, sign at random: one tie over the whole level, decided by index alone."""
    return np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32), "ordered"


def signed_zeros_on_top(rng, n):
    """Negative-only logits with zeros of both signs on top: the zeros tie among themselves inside the top-k."""
    v = -np.abs(rng.normal(5.0, 1.0, n)).astype(F32) - F32(0.5)
    m = min(600, n // 2)
    at = rng.choice(n, size=m, replace=False)
    v[at] = np.where(rng.random(m) < 0.5, F32(0.0), F32(-0.0))
    return v.astype(F32), "fast"


def with_infs(rng, n):
    """Mixed-sign logits with +inf and -inf among them (-inf reaches the top-k where n <= k)."""
    v = rng.normal(0.0, 3.0, n).astype(F32)
    at = rng.choice(n, size=40, replace=False)
    v[at[:20]] = np.inf
    v[at[20:]] = -np.inf
    return v, "fast"


def fast_boundary(in_bin):
    """900 keys in higher bins, `in_bin` distinct keys in the bin [1.0, 1.125), the rest far below: the threshold bin and
    above hold exactly 900 + in_bin keys (3196 -> 4096: the last fast count; 3197 -> 4097: the first general one)."""
    def f(rng, n):
        if n < 900 + in_bin + 100:
            return spread(rng, n)
        v = rng.normal(-8.0, 1.0, n).astype(F32)
        at = rng.choice(n, size=900 + in_bin, replace=False)
        v[at[:900]] = rng.uniform(2.0, 3.0, 900).astype(F32)
        v[at[900:]] = _one_bin_distinct(rng, in_bin)
        v = _tie_pairs_inside_topk(v)                            # (pairs swap values inside their bins: the counts stay)
        return v, ("fast" if 900 + in_bin <= TOPK_FAST else "unordered")
    return f


T_BITS = ONE + BIN_FLOATS // 2          # the tied value of the straddling cases (1.0625)


def _straddle(rng, n, eq_at, n_gt):
    """All keys in the bin [1.0, 1.125): n_gt distinct ones above the tied value, the tied value at eq_at, distinct lower
    ones elsewhere."""
    v = _one_bin_distinct(rng, n, 0, BIN_FLOATS // 2)                 # below the tie
    rest = np.setdiff1d(np.arange(n), eq_at)
    gt_at = rng.choice(rest, size=n_gt, replace=False)
    v[gt_at] = _one_bin_distinct(rng, n_gt, BIN_FLOATS // 2 + 1, BIN_FLOATS)
    v[eq_at] = np.uint32(T_BITS).view(F32)
    return v


def straddle_mid(rng, n):
    """600 keys above a 3000-fold tie; the 400 winners are its lowest indices, and the last of them sits at lane 37 of a
    wave, position 549 of a 1024-key round, with two losers right behind it in the same wave."""
    if n <= TOPK_FAST + ROUND:
        return spread(rng, n)
    last = (n // 2 // ROUND) * ROUND + 549
    lo = rng.choice(last, size=399, replace=False)
    hi = last + 3 + rng.choice(n - last - 3, size=2598, replace=False)
    eq_at = np.concatenate([lo, [last, last + 1, last + 2], hi])
    return _straddle(rng, n, eq_at, K - 400), "ordered"


def straddle_last_round(rng, n):
    """930 keys above a 150-fold tie that lies wholly in the last, partial round of the level; 70 of the 150 win."""
    if n <= TOPK_FAST + ROUND:
        return spread(rng, n)
    start = (n // ROUND) * ROUND
    assert n - start >= 160
    eq_at = start + np.sort(rng.choice(n - start, size=150, replace=False))
    return _straddle(rng, n, eq_at, K - 70), "ordered"


# ---- delta families --------------------------------------------------------------------------------------------------
def zero_deltas(rng, n):
    return np.zeros((n, 4), dtype=F32)


def mixed_deltas(rng, n):
    """Per anchor one of: small random (60 %), dw / dh beyond the clamp log(1000/16) (15 %), a shift that leaves the image
    (15 %; dw = dh = 0), NaN (5 %), +-inf (5 %)."""
    d = rng.normal(0.0, 0.2, (n, 4)).astype(F32)
    kind = rng.random(n)
    big = (kind >= 0.60) & (kind < 0.75)
    d[big] = 0.0
    d[big, 2:] = rng.uniform(4.2, 12.0, (int(big.sum()), 2)).astype(F32)
    out = (kind >= 0.75) & (kind < 0.90)
    d[out] = 0.0
    d[out, :2] = (rng.choice([-1.0, 1.0], (int(out.sum()), 2)) * rng.uniform(80.0, 400.0, (int(out.sum()), 2))).astype(F32)
    nan = (kind >= 0.90) & (kind < 0.95)
    d[nan, rng.integers(0, 4, int(nan.sum()))] = np.nan
    inf = kind >= 0.95
    d[inf, rng.integers(0, 4, int(inf.sum()))] = (rng.choice([-1.0, 1.0], int(inf.sum())) * np.inf).astype(F32)
    return d


def all_outside_deltas(rng, n):
    """Every box is pushed past the right / bottom edge: empty after clipping, so the image ends with no proposal."""
    d = np.zeros((n, 4), dtype=F32)
    d[:, :2] = rng.uniform(100.0, 300.0, (n, 2)).astype(F32)
    return d


# ---- cases -------------------------------------------------------------------------------------------------------------
# name -> map size, per image (logit family, delta family), premises checked by tests/test_rpn_cases.py:
#   survivors per image: ">" more than POST_K boxes survive the per-level NMS, "<" fewer (but some), "0" none, None: no claim
#   boundary per image: the exact count of keys in the threshold bin and above on p2..p4
# The straddle and fast-boundary families need room for a general path: on the levels too small for one (p5, p6 everywhere;
# straddles also need n > 5120) they hand back plain `spread` logits, and the printed intent says "fast" there.
# Equal scores ACROSS levels, which the merge must order by level-major candidate index, come from spread_eighths (a few
# dozen values shared by all five levels), all_equal, signed_zeros_all and near_constant_512ths. The one image with fewer
# than POST_K survivors ("<") gets there through its small valid corner (200 x 120 px), not through its deltas: most of its
# top-k anchors are empty after clipping.
SPECS: Dict[str, dict] = {
    "spread-800x800": dict(size="800x800", images=[(spread, zero_deltas), (spread_eighths, zero_deltas)], survivors=[">", "<"],
                           hw_valid=[(800, 800), (200, 120)]),       # image 1: most top-k anchors lie outside the valid corner
    "spread-800x1344": dict(size="800x1344", images=[(spread_eighths, zero_deltas), (spread, zero_deltas)], survivors=[">", ">"]),
    "near-constant-800x800": dict(size="800x800", images=[(near_constant, mixed_deltas), (near_constant_512ths, mixed_deltas)],
                                  survivors=[None, None]),
    "near-constant-800x1344": dict(size="800x1344", images=[(near_constant_512ths, zero_deltas), (near_constant, zero_deltas)],
                                   survivors=[">", ">"]),
    "all-equal-800x1344": dict(size="800x1344", images=[(all_equal(0.5), zero_deltas), (all_equal(-2.0), zero_deltas)],
                               survivors=[None, None]),
    "straddle-800x800": dict(size="800x800", images=[(straddle_mid, zero_deltas), (straddle_last_round, zero_deltas)],
                             survivors=[None, None]),
    "straddle-800x1344": dict(size="800x1344", images=[(straddle_last_round, zero_deltas), (straddle_mid, mixed_deltas)],
                              survivors=[None, None]),
    "fast-boundary-800x800": dict(size="800x800", images=[(fast_boundary(3196), zero_deltas), (fast_boundary(3197), zero_deltas)],
                                  survivors=[None, None], boundary=[4096, 4097]),
    "signed-zeros-800x800": dict(size="800x800", images=[(signed_zeros_on_top, zero_deltas), (signed_zeros_all, zero_deltas)],
                                 survivors=[None, None]),
    "infs-800x1344": dict(size="800x1344", images=[(with_infs, zero_deltas), (mixed_sign, mixed_deltas)], survivors=[None, None]),
    "negative-800x800": dict(size="800x800", images=[(negative_near_constant, mixed_deltas), (negative_near_constant, zero_deltas)],
                             survivors=[None, ">"]),
    "no-proposals-800x1344": dict(size="800x1344", images=[(spread, mixed_deltas), (spread, all_outside_deltas)],
                                  survivors=[None, "0"]),
    "batch8-800x800": dict(size="800x800",
                           images=[(spread, zero_deltas), (near_constant, zero_deltas), (near_constant_512ths, zero_deltas),
                                   (all_equal(1.25), zero_deltas), (fast_boundary(3197), zero_deltas), (signed_zeros_all, zero_deltas),
                                   (negative_near_constant, zero_deltas), (spread_eighths, zero_deltas)],
                           hw_valid=[(800, 800), (750, 620), (800, 533), (533, 800), (640, 640), (800, 800), (427, 640), (800, 799)],
                           survivors=[None] * 8),
}
CASE_NAMES = list(SPECS)


def make_case(name: str) -> dict:
    """→ dict(name, size (hp, wp), hw_valid [B], feat_hw [5], logits [5] of [B, n_l], deltas [5] of [B, n_l, 4],
    intent [B][5], zero_deltas [B], survivors [B], boundary [B] or None). Deterministic per name."""
    spec = SPECS[name]
    hp, wp = SIZES[spec["size"]]
    feat_hw = level_shapes(hp, wp)
    images = spec["images"]
    B = len(images)
    rng = np.random.default_rng(CASE_NAMES.index(name) + 20250)
    logits = [np.empty((B, h * w * A), dtype=F32) for h, w in feat_hw]
    deltas = [np.empty((B, h * w * A, 4), dtype=F32) for h, w in feat_hw]
    intent = []
    for b, (lf, df) in enumerate(images):
        row = []
        for l, (h, w) in enumerate(feat_hw):
            n = h * w * A
            v, want = lf(rng, n)
            assert v.dtype == F32 and v.shape == (n,)
            logits[l][b] = v
            deltas[l][b] = df(rng, n)
            row.append(want if n > TOPK_FAST else "fast")       # a level of <= 4096 anchors can only take the fast path
        intent.append(row)
    return dict(name=name, size=(hp, wp), hw_valid=list(spec.get("hw_valid", HW_VALID[spec["size"]])), feat_hw=feat_hw,
                logits=logits, deltas=deltas, intent=intent, zero_deltas=[df is zero_deltas for _, df in images],
                survivors=list(spec["survivors"]), boundary=spec.get("boundary"))


def head_arrays(case: dict) -> List[np.ndarray]:
    """The five fused head tensors [B, h, w, 15] the engine keeps: 3 logits, then 12 deltas per position."""
    out = []
    for (h, w), lg, dl in zip(case["feat_hw"], case["logits"], case["deltas"]):
        B = lg.shape[0]
        out.append(np.ascontiguousarray(np.concatenate([lg.reshape(B, h, w, A), dl.reshape(B, h, w, A * 4)], axis=3), dtype=F32))
    return out
