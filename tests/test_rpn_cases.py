"""CPU proof that tests/rpn_cases.py covers what tests/test_rpn_select_gpu.py claims: every case lands, per image and
level, on the code path of rpn_topk_decode_kernel it intends (``regime``: the dispatch rule restated in numpy, not the
library), the oracle runs on it, and the case's own premises hold. Prints the regime and candidate count of every image
and level. A path counts as covered only if it appears on p2 and on p3 at both map sizes."""
import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from oracle.maskrcnn_ref import MaskRCNNOracle
from tests import rpn_cases as rc


def test_key_order_and_regime_on_known_inputs():
    v = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, 1.0, 1.124, 1.125, np.inf], dtype=np.float32)
    k = rc.float_to_key(v)
    assert k[3] == k[4] == 0x80000000                                        # the two zeros share a key
    assert (np.diff(k.astype(np.int64))[[0, 1, 2, 4, 5, 6, 7, 8, 9]] > 0).all()
    assert (k[7] >> 20) == (k[8] >> 20) != (k[9] >> 20)                      # [1.0, 1.125) is one coarse bin
    rng = np.random.default_rng(0)
    # 4096 keys in the threshold bin and above: fast; one more: general. k-th key unique: unordered; tied across the cut: ordered
    low = rng.normal(-8, 1, 20000).astype(np.float32)
    a = np.concatenate([rc._one_bin_distinct(rng, 4096), low])
    assert rc.regime(a, 1000) == ("fast", 4096)
    b = np.concatenate([rc._one_bin_distinct(rng, 4097), low])
    assert rc.regime(b, 1000) == ("unordered", 4097)
    c = b.copy()
    top = np.argsort(-c)[:1002]
    c[top[998:1002]] = c[top[998]]                                           # a 4-fold tie at ranks 999..1002
    assert rc.regime(c, 1000) == ("ordered", 4097)
    c[top[998:1002]] = b[top[998:1002]]
    c[top[996:1000]] = c[top[996]]                                           # the tie ends exactly at the cut
    assert rc.regime(c, 1000) == ("unordered", 4097)
    assert rc.regime(np.zeros(5000, np.float32), 1000) == ("ordered", 5000)
    assert rc.regime(np.zeros(507, np.float32), 1000) == ("fast", 507)       # k = n
    assert rc.regime(np.array([-0.0, 0.0, -0.0, 0.0] * 2000, np.float32), 1000) == ("ordered", 8000)


def test_level_shapes_are_the_production_maps():
    assert rc.level_shapes(800, 800) == [(200, 200), (100, 100), (50, 50), (25, 25), (13, 13)]
    assert rc.level_shapes(800, 1344) == [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    assert 200 * 200 * rc.A == 120000 and 200 * 336 * rc.A == 201600


def _level_nms(tap, level):
    m = tap["cand_lvl"] == level
    return R.nms(tap["cand_boxes"][m], tap["cand_scores"][m], 0.7)


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_reaches_what_it_intends(name, capsys):
    case = rc.make_case(name)
    B = len(case["hw_valid"])
    assert B == (8 if name.startswith("batch8") else 2)
    lines = []
    for b in range(B):
        assert case["hw_valid"][b][0] <= case["size"][0] and case["hw_valid"][b][1] <= case["size"][1]
        for l in range(5):
            lg = case["logits"][l][b]
            assert not np.isnan(lg).any()
            got, cand = rc.regime(lg, rc.K)
            lines.append(f"  {name} image {b} p{l + 2}: {got} ({cand} keys in the threshold bin and above, {lg.size} anchors)")
            assert got == case["intent"][b][l], lines[-1]
            if case["boundary"] is not None and l <= 2:
                assert cand == case["boundary"][b], lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    if case["boundary"] is not None:
        assert case["intent"][0][:3] == ["fast"] * 3 and case["intent"][1][:3] == ["unordered"] * 3
    # the oracle runs on the case; premises about its result
    logits = [torch.from_numpy(a) for a in case["logits"]]
    deltas = [torch.from_numpy(a) for a in case["deltas"]]
    with np.errstate(all="ignore"):
        props, taps = MaskRCNNOracle({}).rpn_proposals(logits, deltas, case["feat_hw"], case["hw_valid"])
    for b in range(B):
        boxes, scores = props[b]
        assert np.isfinite(boxes).all() and np.isfinite(scores).all()
        want = case["survivors"][b]
        if want == ">":
            total = sum(len(_level_nms(taps[b], l)) for l in range(5))
            assert total > rc.POST_K and len(boxes) == rc.POST_K, (name, b, total)
        elif want == "<":
            assert 0 < len(boxes) < rc.POST_K, (name, b, len(boxes))
        elif want == "0":
            assert len(boxes) == 0 and len(taps[b]["cand_scores"]) == 0, (name, b, len(boxes))
        for l in range(5):
            assert len(taps[b]["per_level"][l]["topk_idx"]) == min(rc.K, case["logits"][l].shape[1])
    if name.startswith("infs"):
        s = taps[0]["per_level"][0]["topk_scores"]
        assert np.isposinf(s[:20]).all() and np.isfinite(s[20:]).all()            # +inf wins the top-k and is dropped after it
        assert np.isneginf(taps[0]["per_level"][4]["topk_scores"][-20:]).all()    # p6: k = n, -inf is among the candidates
    if name.startswith("signed-zeros"):
        s = taps[0]["per_level"][0]["topk_scores"]
        z = s == 0
        assert z[:600].all() and not z[600:].any() and np.signbit(s[:600]).any() and not np.signbit(s[:600]).all()
        assert (np.diff(taps[0]["per_level"][0]["topk_idx"][:600]) > 0).all()     # zeros of either sign: by index alone
        assert np.array_equal(taps[1]["per_level"][0]["topk_idx"], np.arange(rc.K))
    if name.startswith("straddle"):
        tie = np.uint32(rc.T_BITS).view(np.float32)
        for b, fam in enumerate(rc.SPECS[name]["images"]):
            for l in range(3):
                lg, idx = case["logits"][l][b], taps[b]["per_level"][l]["topk_idx"]
                winners = idx[lg[idx] == tie]
                eq_at = np.nonzero(lg == tie)[0]
                assert np.array_equal(winners, eq_at[: len(winners)]) and len(winners) < len(eq_at)
                if fam[0] is rc.straddle_mid:
                    last = int(winners[-1])
                    assert len(winners) == 400 and last % 64 == 37 and last % rc.ROUND == 549
                    assert lg[last + 1] == tie and lg[last + 2] == tie                 # losers right behind, same wave
                else:
                    assert len(winners) == 70 and eq_at.min() >= (lg.size // rc.ROUND) * rc.ROUND


def test_every_path_is_reached_on_p2_and_p3_at_both_sizes():
    seen = set()
    for name in rc.CASE_NAMES:
        case = rc.make_case(name)
        for b in range(len(case["hw_valid"])):
            for l in range(5):
                seen.add((rc.regime(case["logits"][l][b], rc.K)[0], l, case["size"]))
    for path in ("fast", "unordered", "ordered"):
        for l in (0, 1):
            for size in rc.SIZES.values():
                assert (path, l, size) in seen, (path, f"p{l + 2}", size)
