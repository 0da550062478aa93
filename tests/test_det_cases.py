"""CPU proof that tests/det_cases.py covers what tests/test_det_select_gpu.py and tests/test_mask_tail_gpu.py claim: with
the oracle alone (MaskRCNNOracle.detections / .postprocess, R.nms, R.apply_deltas, R.clip_boxes) every image of every case
reaches what its tags and ``expect`` say, and the rows the oracle-selection comparison may leave out (float64 score within
the derived tolerance of the threshold) are only rows crafted to sit there. Prints, per case, how many rows are compared
exactly and how many within a tolerance."""
import numpy as np
import pytest

from oracle import ops_ref as R
from tests import det_cases as dc


def iou(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    i = w * h
    return i / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - i)


def test_score_reference_and_bound_on_known_inputs():
    assert dc.softmax64(0.0, 0.0) == 0.5 and dc.softmax64(3e38, 3e38) == 0.5
    assert dc.softmax64(0.0, -np.inf) == 1.0 and dc.softmax64(-np.inf, 0.0) == 0.0
    assert np.isnan(dc.softmax64(np.inf, 0.0)) and np.isnan(dc.softmax64(-np.inf, -np.inf)) and np.isnan(dc.softmax64(np.nan, 0.0))
    assert abs(dc.softmax64(dc.T03, 0.0) - 0.3) < 1e-15
    # at 0.5 with d = 0: (2 * 2u + 2u) / 2 = 3u; the bound grows with |d|; exact classes have no slack
    assert abs(dc.score_tol(dc.step(1.0, 1), 1.0) - 3 * dc.U) < 1e-13 and dc.score_tol(1.0, 1.0) == 0.0
    assert dc.score_tol(0.0, -np.inf) == 0.0 and dc.score_tol(-np.inf, 0.0) == 0.0
    assert dc.score_tol(3e38, -3e38) == 2.0 ** -148 and dc.score_tol(5.0, 0.0) > dc.score_tol(1.0, 0.0) * 0.99
    assert dc.step(1.0, 1) == np.float32(1.0) + np.float32(2.0 ** -23) and dc.step(1.0, -1) == np.float32(1.0 - 2.0 ** -24)
    a, c = dc.border_ulp_box(60)
    box = R.clip_boxes(R.apply_deltas(np.zeros((1, 4), np.float32), np.array([[a, 1, c, 3]], np.float32), (10, 10, 5, 5)), 50, 60)[0]
    assert box[2] == 60 and box[0] == np.nextafter(np.float32(60), np.float32(0))


def test_batch_geometry_is_what_the_stage_tests_need():
    assert len(dc.HW_VALID) == len(dc.HW_OUT) == 3 and len(set(dc.HW_VALID)) == 3 and len(set(dc.HW_OUT)) == 3
    assert all(h <= dc.SIZE[0] and w <= dc.SIZE[1] for h, w in dc.HW_VALID)
    assert any(h % 32 or w % 32 for h, w in dc.HW_OUT)
    ratio = [(o[0] / v[0], o[1] / v[1]) for v, o in zip(dc.HW_VALID, dc.HW_OUT)]
    assert any(a > 1 and b > 1 for a, b in ratio) and any(a < 1 and b < 1 for a, b in ratio)


@pytest.mark.parametrize("name", dc.CASE_NAMES + dc.MASK_CASE_NAMES)
def test_case_reaches_what_it_intends(name, capsys):
    case = dc.make_case(name)
    P, thr = case["P"], np.float32(case["thresh"])
    B = len(case["hw_valid"])
    assert B == 3 and case["props"].shape == (B, P, 4) and case["box_pred"].shape == (B * P, 6)
    pred_all = case["box_pred"].reshape(B, P, 6)
    lines = []
    for b in range(B):
        n = int(case["count"][b])
        at = (name, b)
        assert 0 <= n <= P, at
        assert np.isnan(pred_all[b, n:, 2:]).all() and (pred_all[b, n:, 0] == np.float32(1e30)).all(), at     # poison beyond the count
        pred, tags, exp = pred_all[b, :n], np.asarray(case["tags"][b], dtype=object), case["expect"][b]
        o = dc.oracle_image(case, b)
        assert np.isfinite(o["final_boxes"]).all() and np.isfinite(o["final_scores"]).all(), at
        assert len(o["final_scores"]) <= dc.D
        # ---- which rows are compared how
        excluded = dc.excluded_rows(case, b)
        assert not (excluded & ~case["near"][b]).any(), (at, "a row not crafted to sit at the threshold is within the tolerance of it",
                                                         np.nonzero(excluded & ~case["near"][b])[0])
        zero = (pred[:, 2:] == 0).all(axis=1) if n else np.zeros(0, bool)
        fin_box = np.isfinite(o["decoded"]).all(axis=1) if n else np.zeros(0, bool)
        s64 = dc.softmax64(pred[:, 0], pred[:, 1])
        tol = dc.score_tol(pred[:, 0], pred[:, 1])
        lines.append(f"  {name} image {b}: {n} live rows | flags exact vs the engine's score: {n} | flags vs the oracle: {n - int(excluded.sum())} "
                     f"({int(excluded.sum())} within the score tolerance of {float(thr)}) | scores exact class (tolerance 0 or NaN): "
                     f"{int((~np.isfinite(s64) | (tol == 0)).sum())}, within tolerance: {int((np.isfinite(s64) & (tol > 0)).sum())} | boxes exact: "
                     f"{int((zero & fin_box).sum())}, within {dc.TOL_BOX} px: {int((~zero & fin_box).sum())}, non-finite: {int((~fin_box).sum())} "
                     f"| selected {int(o['sel'].sum())}, after NMS {len(o['nms_rows'])}, final {len(o['final_rows'])}")
        if "count" in exp:
            assert len(o["final_rows"]) == exp["count"], (at, len(o["final_rows"]))
        if exp.get("no_proposals"):
            assert n == 0, at
        if exp.get("live"):
            assert len(o["final_rows"]) > 0 and (~o["sel"]).any(), at
        if exp.get("both_sides"):
            f = np.isfinite(s64)
            assert (o["sel"] & f).any() and (~o["sel"] & f).any(), at
            st = np.array([t.startswith("step") for t in tags])
            assert not st.any() or ((o["sel"] & st).any() and (~o["sel"] & st).any()), at   # the stepped rows fall on both sides too
        if "on" in exp:
            on = tags == "on"
            assert int(on.sum()) == exp["on"] >= 1, at
            assert (o["scores"][on] == np.float32(0.5)).all() and (s64[on] - 0.5 <= 1e-40).all() and thr == np.float32(0.5), at
            assert not o["sel"][on].any() and excluded[on].all(), at                  # exactly on the threshold: dropped by the strict >
        if exp.get("nonfinite"):
            _nonfinite_premises(at, case, b, o, pred, tags)
        if "kept_rows" in exp:
            assert np.array_equal(o["kept_rows"], exp["kept_rows"]), (at, o["kept_rows"][:12])
            assert len(np.unique(o["scores"][o["sel"]].view(np.uint32))) <= 2, at      # bit-equal scores
            if "survivors" in exp:
                assert len(o["nms_rows"]) == exp["survivors"], at
        if "chains" in exp:
            _chain_premises(at, case, b, o, exp)
        if exp.get("survivors_gt_D"):
            _over_d_premises(at, case, b, o, exp, tags)
        if name.startswith("mask"):
            assert np.array_equal(o["final_rows"], np.arange(exp["count"])), at      # one score, disjoint: detection d is row d
    if name == "p130":
        assert P == 130 and P % 64 != 0
    if name == "mask-7-0-100":
        fb = dc.oracle_image(case, 0)["final_boxes"]
        oh, ow = case["hw_out"][0]
        assert np.array_equal(fb[0], [0, 0, ow, oh])                                  # touches all four borders
        assert 0 < fb[1, 2] - fb[1, 0] < 1 and 0 < fb[1, 3] - fb[1, 1] < 1            # under one pixel
        assert fb[2, 0] == 0 and fb[3, 2] == ow and fb[4, 1] == 0 and fb[5, 3] == oh  # one on each border
        widths = [R.paste_region(x, oh, ow)[2] - R.paste_region(x, oh, ow)[0] for x in fb]
        assert any(w > 32 and w % 32 for w in widths), widths                         # a partial last word after a full one
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def _nonfinite_premises(at, case, b, o, pred, tags):
    hw = case["hw_valid"][b]
    row = lambda t: int(np.nonzero(tags == t)[0][0])
    for c in range(6):
        r = row(f"col{c}=nan")
        assert not o["sel"][r] and not o["finite"][r], (at, c)                        # NaN anywhere: dropped
    for c in (2, 3):
        for v in ("inf", "-inf"):
            assert not o["finite"][row(f"col{c}={v}")], (at, c, v)                    # an infinite shift: dropped
    assert np.isnan(o["scores"][row("col0=inf")]) and np.isnan(o["scores"][row("col1=inf")]), at
    assert o["scores"][row("col0=-inf")] == 0 and not o["sel"][row("col0=-inf")], at
    assert o["scores"][row("col1=-inf")] == 1 and o["sel"][row("col1=-inf")], at
    assert not o["finite"][row("both-logits--inf")] and not o["finite"][row("both-logits-+inf")], at
    clamp = float(R.SCALE_CLAMP)
    for r in list(np.nonzero(tags == "clamp")[0]) + [row("col4=inf"), row("col5=inf")]:
        d = pred[r, 2:].astype(np.float64)
        assert max(d[2], d[3]) / 5.0 > clamp and o["finite"][r] and o["sel"][r], (at, r)    # clamped, finite, kept
        wh = case["props"][b, r, 2:] - case["props"][b, r, :2]
        got = o["decoded"][r, 2:] - o["decoded"][r, :2]
        want = np.exp(np.minimum(d[2:] / 5.0, clamp)) * wh
        assert np.abs(got - want).max() < 1e-3 * want.max(), (at, r)                 # the box of the clamped scale
        assert (o["boxes"][r] >= 0).all() and o["boxes"][r, 2] <= hw[1] and o["boxes"][r, 3] <= hw[0], at
    r = row("clamp-small")                                                         # clamped and NOT clipped: the constant is visible
    d = pred[r, 2:].astype(np.float64)
    assert min(d[2], d[3]) / 5.0 > clamp and o["finite"][r] and o["sel"][r] and r in o["final_rows"], at
    wh = (case["props"][b, r, 2:] - case["props"][b, r, :2]).astype(np.float64)
    got = (o["decoded"][r, 2:] - o["decoded"][r, :2]).astype(np.float64)
    assert np.abs(got - 62.5 * wh).max() < 1e-4 and np.array_equal(o["boxes"][r], o["decoded"][r]), (at, got)
    assert (o["boxes"][r, :2] > 1).all() and o["boxes"][r, 2] < hw[1] - 1 and o["boxes"][r, 3] < hw[0] - 1, at
    for c in (4, 5):
        r = row(f"col{c}=-inf")                                                    # exp(-inf) = 0: a zero-extent box, finite, selected,
        assert o["finite"][r] and o["sel"][r] and r not in o["final_rows"], (at, c)   # dropped as empty by the postprocess
    for r in np.nonzero(tags == "overflow")[0]:
        assert np.isfinite(pred[r]).all() and not o["finite"][r] and not o["sel"][r], (at, r)
    for r in np.nonzero(tags == "score-1")[0]:
        assert o["scores"][r] == np.float32(1.0) and o["sel"][r], (at, r)            # exactly 1.0 is kept


def _chain_premises(at, case, b, o, exp):
    assert int(o["sel"].sum()) == exp["passing"], at
    sel_rows = np.nonzero(o["sel"])[0]
    assert len(np.unique(o["scores"][sel_rows].view(np.uint32))) == 1, at          # one score: sorted by index
    pos = {int(r): p for p, r in enumerate(sel_rows)}
    kept = set(int(r) for r in o["nms_rows"])
    crossing = 0
    for rows, want_pos in zip(exp["chains"], exp["chain_pos"]):
        assert tuple(pos[r] for r in rows) == tuple(want_pos), (at, rows)
        bx = [o["boxes"][r] for r in rows]
        assert rows[0] in kept and rows[1] not in kept and iou(bx[0], bx[1]) > 0.52, (at, rows)
        if len(rows) == 3:
            assert rows[2] in kept and iou(bx[1], bx[2]) > 0.52 and iou(bx[0], bx[2]) < 0.3, (at, rows)   # B would have suppressed C
        chunks = [p // 64 for p in want_pos]
        crossing += len(set(chunks)) == len(chunks)
    if exp["passing"] >= 65:
        assert crossing >= 1, at                                                     # members in different 64-box chunks
    if exp["passing"] >= 129:
        assert any(len(c) == 3 and len({p // 64 for p in c}) == 3 for c in exp["chain_pos"]), at
    assert len(kept) == exp["passing"] - len(exp["chains"]), at


def _over_d_premises(at, case, b, o, exp, tags):
    assert len(o["nms_rows"]) > dc.D and np.array_equal(o["kept_rows"], np.arange(dc.D)), at
    final = o["final_rows"]
    empties = [r for r in range(dc.D) if tags[r] in ("clip-empty", "ulp-merge")]
    assert len(empties) == exp["empties_in_first_D"] and len(final) == dc.D - len(empties), at
    assert np.array_equal(final, [r for r in range(dc.D) if r not in empties]), at    # compacted, nothing refilled from rank 101 on
    for r in np.nonzero(tags == "ulp-merge")[0]:
        net = o["boxes"][r]                                                           # one ulp wide before the scaling: kept by the NMS
        assert net[2] - net[0] > 0 and net[2] == np.nextafter(net[0], np.float32(np.inf)) and r in o["kept_rows"], (at, r)
        sx = np.float32(case["hw_out"][b][1] / case["hw_valid"][b][1])
        assert np.float32(net[0] * sx) == np.float32(net[2] * sx) and r not in final, (at, r)    # the edges merge in the scaling
    assert (tags == "ulp-merge").sum() == (2 if (case["name"], b) == ("over_D", 1) else 0), at
    if case["name"] == "over_D" and b < 2:
        assert len(empties) >= 2 and len(final) < dc.D, at
