"""The detection-selection stage (roi.hip: det_decode_kernel, det_finalize_kernel; rpn.hip: sort_boxes_kernel,
nms_mask_kernel, nms_scan_kernel with device-side counts and max_keep = D) on the crafted box-head outputs of
tests/det_cases.py, against oracle/maskrcnn_ref.py and oracle/ops_ref.py. tests/test_det_cases.py proves on the CPU that
every case reaches what it intends; tests/det_stage.py overwrites ``proposals`` / ``proposal_count`` / ``box_pred`` between
phases 2 and 3 and poisons every buffer the stage writes. Every image and every live row of every case is checked:

  * det_all_scores: NaN exactly where the float64 softmax of the crafted logits is NaN, else within det_cases.score_tol
    (derived there: two expf of at most 1 ulp — the HIP math API's documented bound, assumed: the document is not shipped
    with the toolchain —, a rounded argument, one add, one divide; 0 for l0 == l1 and for an infinite difference);
  * det_flags: equal to finite(row) && score > thresh evaluated on the engine's OWN read-back score, for every live row
    without exception. Only the score half of that is the engine's: finite(row) takes the box half from the ORACLE's
    float32 decode of the row (R.apply_deltas finite; det_all_boxes holds clipped values, from which an overflow can no
    longer be read), which is sound because the crafted rows overflow by many orders of magnitude or not at all; the
    score half is finite(score) and finite(1 - score) of the read-back score;
    equal to the oracle's selection for every row whose float64 score is farther from the threshold than that tolerance
    (the rows left out are counted; test_det_cases.py proves they are only rows crafted to sit there); rows with
    l0 == l1 under the 0.5 engine are 0;
  * det_all_boxes: rows with zero deltas (exp(0) = 1: the decode is exact) equal to the oracle's clipped boxes, others,
    the clamped dw / dh rows included (one of them on a sub-pixel proposal, so that its 31 x 25 px box is not clipped and
    shows the clamp constant itself), within TOL_BOX = 1e-3 px of them (what test_rpn_select_gpu.py grants expf);
  * beyond proposal_count: flags, scores and boxes are 0;
  * det_sorted_* / det_keep / det_keep_count: the flagged rows by (score descending, index ascending); R.nms(.., 0.5) on
    the engine's own flagged boxes and scores, cut to D, exactly;
  * out boxes / scores / classes / count and det_boxes_net: MaskRCNNOracle.postprocess(paste=False) of those kept rows,
    exactly, compacted identically, classes 0, zeros beyond the count;
  * images whose live rows all have zero deltas: the oracle's detections + postprocess end to end — the same rows in the
    same order, boxes and count bit-equal, scores bit-equal where the softmax is exact (0.5, 1.0) and otherwise bit-equal
    to the engine's own score of the row the oracle picked (see ``end_to_end``); images with other deltas: the same rows,
    boxes within TOL_BOX.
"""
import numpy as np
import pytest

from oracle import ops_ref as R
from oracle.maskrcnn_ref import MaskRCNNOracle
from tests import det_cases as dc
from tests.det_stage import make_engine, run_stage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_for():
    """The three engines of det_cases.ENGINES, built on first use, closed at teardown."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make_engine(kind)
        return made[kind]
    yield get
    for e in made.values():
        e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_selection_matches_the_oracle(name, engine_for):
    case = dc.make_case(name)
    got = run_stage(engine_for(case["engine"]), case)
    P, D, thr = case["P"], dc.D, np.float32(case["thresh"])
    pred_all = case["box_pred"].reshape(3, P, 6)
    assert got["det_all_boxes"].shape == (3, P, 4) and got["det_flags"].shape == (3, P) and got["det_keep"].shape == (3, D)
    assert got["boxes"].shape == (3, D, 4) and got["det_boxes_net"].shape == (3, D, 4)
    assert (got["classes"] == 0).all(), name
    for b in range(3):
        n = int(case["count"][b])
        at = (name, b)
        pred, tags = pred_all[b, :n], case["tags"][b]
        o = dc.oracle_image(case, b)
        g_sc, g_fl, g_bx = got["det_all_scores"][b], got["det_flags"][b], got["det_all_boxes"][b]
        # ---- beyond the count
        assert (g_fl[n:] == 0).all() and (bits(g_sc[n:]) == 0).all() and (bits(g_bx[n:]) == 0).all(), at
        assert np.isin(g_fl, (0, 1)).all(), at
        # ---- scores
        s64 = dc.softmax64(pred[:, 0], pred[:, 1])
        tol = dc.score_tol(pred[:, 0], pred[:, 1])
        assert np.array_equal(np.isnan(g_sc[:n]), np.isnan(s64)), (at, "NaN scores", np.nonzero(np.isnan(g_sc[:n]) != np.isnan(s64))[0])
        f = np.isfinite(s64)
        err = np.abs(g_sc[:n][f].astype(np.float64) - s64[f])
        pos = tol[f] > 0
        print(f"{at}: scores: {int((~f).sum())} NaN rows, {int((~pos).sum())} rows of tolerance 0, {int(pos.sum())} within tolerance, "
              f"max error / bound {float((err[pos] / tol[f][pos]).max()) if pos.any() else 0.0:.3f}")
        bad = err > tol[f]
        assert not bad.any(), (at, "scores", np.nonzero(f)[0][bad][:8], g_sc[:n][f][bad][:8], s64[f][bad][:8], tol[f][bad][:8])
        # ---- flags: exact against the engine's own score, every live row
        with np.errstate(all="ignore"):
            fin_row = np.isfinite(o["decoded"]).all(axis=1) & np.isfinite(g_sc[:n]) & np.isfinite(np.float32(1) - g_sc[:n])
            want = fin_row & (g_sc[:n] > thr)
        diff = (g_fl[:n] > 0) != want
        assert not diff.any(), (at, "flags vs own score", [(int(r), tags[r], pred[r].tolist(), float(g_sc[r])) for r in np.nonzero(diff)[0][:6]])
        # ---- flags: the oracle's selection wherever the score tolerance cannot move the decision
        excluded = dc.excluded_rows(case, b)
        diff = ((g_fl[:n] > 0) != o["sel"]) & ~excluded
        assert not diff.any(), (at, "flags vs oracle", [(int(r), tags[r], pred[r].tolist(), float(g_sc[r])) for r in np.nonzero(diff)[0][:6]])
        print(f"{at}: flags exact on {n} rows; against the oracle on {n - int(excluded.sum())}, {int(excluded.sum())} left out")
        on = np.array([t == "on" for t in tags], dtype=bool)
        if on.any():
            assert (g_sc[:n][on] == np.float32(0.5)).all() and (g_fl[:n][on] == 0).all(), at     # exactly 0.5 is not > 0.5
        # ---- boxes
        fin_box = np.isfinite(o["decoded"]).all(axis=1)
        zero = (pred[:, 2:] == 0).all(axis=1)
        ex = fin_box & zero
        assert np.array_equal(bits(g_bx[:n][ex]), bits(o["boxes"][ex])), (at, "boxes of zero-delta rows")
        ap = fin_box & ~zero
        if ap.any():
            e = np.abs(g_bx[:n][ap] - o["boxes"][ap]).max(axis=1)
            print(f"{at}: box error max {float(e.max()):.3g} px over {int(ap.sum())} rows")
            assert (e < dc.TOL_BOX).all(), (at, [(int(r), tags[r]) for r in np.nonzero(ap)[0][e >= dc.TOL_BOX][:6]])
        # ---- sort: flagged rows by (score descending, index)
        idx = np.nonzero(g_fl[:n])[0]
        order = idx[R.stable_desc_order(g_sc[idx])]
        m = len(order)
        assert got["det_sorted_count"][b] == m, at
        assert np.array_equal(bits(got["det_sorted_scores"][b, :m]), bits(g_sc[order])), (at, "sorted scores")
        assert np.array_equal(bits(got["det_sorted_boxes"][b, :m]), bits(g_bx[order])), (at, "sorted boxes")
        assert (bits(got["det_sorted_scores"][b, m:]) == 0).all() and (bits(got["det_sorted_boxes"][b, m:]) == 0).all(), at
        # ---- NMS on the engine's own flagged boxes and scores, cut to D
        with np.errstate(all="ignore"):
            keep_all = R.nms(g_bx[order], g_sc[order], dc.NMS_THR)        # positions in the sorted list (already sorted: stable)
        keep = keep_all[:D]
        assert got["det_keep_count"][b] == len(keep) == min(len(keep_all), D), (at, int(got["det_keep_count"][b]), len(keep_all))
        assert np.array_equal(got["det_keep"][b, : len(keep)], keep), (at, "keep list")
        # ---- finalize: scale, clip, drop empties, compact
        kb, ks = g_bx[order][keep], g_sc[order][keep]
        fb, fs, fr, _ = MaskRCNNOracle.postprocess(kb, ks, np.arange(len(keep)), case["hw_valid"][b], case["hw_out"][b], paste=False)
        c = int(got["count"][b])
        assert c == len(fs), (at, c, len(fs))
        assert np.array_equal(bits(got["boxes"][b, :c]), bits(fb)) and np.array_equal(bits(got["scores"][b, :c]), bits(fs)), at
        assert np.array_equal(bits(got["det_boxes_net"][b, :c]), bits(kb[fr])), (at, "det_boxes_net")
        assert (bits(got["boxes"][b, c:]) == 0).all() and (bits(got["scores"][b, c:]) == 0).all(), at
        assert (bits(got["det_boxes_net"][b, c:]) == 0).all(), at
        # ---- the oracle end to end
        end_to_end(at, case, b, o, got, order[keep][fr], bool(zero.all()), excluded)
        exp = case["expect"][b]
        if "count" in exp:
            assert c == exp["count"], (at, c)
        if exp.get("survivors_gt_D"):
            assert len(keep_all) > D and c < D + (exp["empties_in_first_D"] == 0), at
        if "kept_rows" in exp:
            assert np.array_equal(order[keep], exp["kept_rows"]), at


def end_to_end(at, case, b, o, got, final_rows, all_zero_deltas, excluded):
    """The engine's final rows against the oracle's detections + postprocess of the crafted inputs. Rows within the score
    tolerance of the threshold (``excluded``; they are disjoint from every other box and the images that hold them keep
    fewer than D rows, so they change nothing else) are taken out of both lists; the rest must be the same rows in the
    same order. With zero deltas the boxes are bit-equal, and so are the scores: bit-equal to the oracle's where the
    softmax has no rounding of its own (l0 == l1: 0.5; an infinite difference: 1.0), and for every other row bit-equal to
    the engine's own det_all_scores of the row the oracle picked and within twice score_tol (one for each side) plus one
    rounding of the oracle's float32 value — two exp implementations need not agree to the last bit, and the selection
    does not hang on it, the rows being the same. With other deltas: boxes within TOL_BOX times the output scale."""
    c = int(got["count"][b])
    if excluded.any():
        assert len(o["nms_rows"]) < dc.D and c < dc.D, at
    mine = [int(r) for r in final_rows if not excluded[r]]
    theirs = [int(r) for r in o["final_rows"] if not excluded[r]]
    assert mine == theirs, (at, "rows", mine[:10], theirs[:10])
    if not excluded.any():
        assert c == len(o["final_rows"]), at
    if not mine:
        return
    gi = np.array([list(final_rows).index(r) for r in mine])
    oi = np.array([list(o["final_rows"]).index(r) for r in mine])
    pred = case["box_pred"].reshape(3, case["P"], 6)[b][mine]
    tol = dc.score_tol(pred[:, 0], pred[:, 1])
    g, ref = got["scores"][b, :c][gi], o["final_scores"][oi]
    assert np.array_equal(bits(g), bits(got["det_all_scores"][b][mine])), at
    exact = tol == 0
    assert np.array_equal(bits(g[exact]), bits(ref[exact])), (at, "scores of exact class")
    print(f"{at}: end to end {len(mine)} rows, scores bit-equal to the oracle's on {int((bits(g) == bits(ref)).sum())}, "
          f"exact class {int(exact.sum())}")
    assert (np.abs(g.astype(np.float64) - ref.astype(np.float64)) <= 2 * tol + 2.0 ** -24 * ref).all(), at
    if all_zero_deltas:
        assert np.array_equal(bits(got["boxes"][b, :c][gi]), bits(o["final_boxes"][oi])), (at, "boxes end to end")
        assert np.array_equal(bits(got["det_boxes_net"][b, :c][gi]), bits(o["boxes"][mine])), at
    else:
        scale = max(case["hw_out"][b][0] / case["hw_valid"][b][0], case["hw_out"][b][1] / case["hw_valid"][b][1], 1.0)
        assert np.abs(got["boxes"][b, :c][gi] - o["final_boxes"][oi]).max() < dc.TOL_BOX * scale, at
