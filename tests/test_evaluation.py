"""treedetection_amd.evaluation on the CPU: the host twin of the two-set box-pair kernel against a numpy brute force, the greedy
matcher on hand-written sparse input and against a dense restatement of the reference's loop, evaluate(device=None) on a grid of
squares with hand-derived scores, and the layer functions on files written into tmp_path. The device side of the same calls:
tests/test_evaluation_gpu.py."""
import ctypes as C
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cases as E  # noqa: E402
import ring_iou_ref as R  # noqa: E402
from treedetection_amd import _lib  # noqa: E402
from treedetection_amd import evaluation as EV  # noqa: E402
from treedetection_amd import gpkg  # noqa: E402


# ---- td_box_pairs_ab ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.box_cases()))
def test_host_box_pairs_equal_the_brute_force(name):
    a, b = E.box_cases()[name]
    got = EV.box_pairs_ab(a, b, device=None)
    want = E.brute_pairs(a, b)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, got[:5], want[:5])
    if name in ("touching_edge", "touching_corner", "0x0", "0x5", "5x0"):
        assert got.shape == (0, 2)
    if name == "identical":
        assert got.shape == (6, 2)
    if name == "nan_slots":
        assert set(got[:, 0].tolist()) == {4, 5} and set(got[:, 1].tolist()) == {0, 1}         # only the boxes without a NaN
    if name in ("257x1025", "700x900"):
        assert got.shape[0] > max(a.shape[0], b.shape[0])                                      # (the case means something)


def test_host_box_pairs_rows_ascend_and_capacity_is_checked():
    a, b = E.box_cases()["700x900"]
    lib = _lib.load()
    counts = np.zeros(len(a), np.int32)
    assert lib.td_box_pairs_ab(a.ctypes.data, len(a), b.ctypes.data, len(b), counts.ctypes.data, None, 0) == 0
    total = int(counts.sum())
    cols = np.full(total + 1, -7, np.int32)
    assert lib.td_box_pairs_ab(a.ctypes.data, len(a), b.ctypes.data, len(b), counts.ctypes.data, cols.ctypes.data, total) == 0
    assert cols[total] == -7
    start = np.concatenate([[0], np.cumsum(counts)])
    assert all((np.diff(cols[start[i]:start[i + 1]]) > 0).all() for i in range(len(a)))
    assert lib.td_box_pairs_ab(a.ctypes.data, len(a), b.ctypes.data, len(b), counts.ctypes.data, cols.ctypes.data, total - 1) == _lib.ERR_CAPACITY
    assert lib.td_box_pairs_ab(None, 1, b.ctypes.data, len(b), counts.ctypes.data, None, 0) == _lib.ERR_INVALID and b"null" in lib.td_last_error()
    assert lib.td_box_pairs_ab(a.ctypes.data, -1, b.ctypes.data, len(b), counts.ctypes.data, None, 0) == _lib.ERR_INVALID
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        EV.box_pairs_ab(np.zeros((3, 3)), b, device=None)


# ---- td_match_greedy ------------------------------------------------------------------------------------------------------------
def csr(rows):
    """[[(annotation, iou), ...] per prediction] → the matrix."""
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [e for r in rows for e in r]
    return row_start, np.array([j for j, _ in flat], np.int32), np.array([v for _, v in flat], np.float64)


def test_an_earlier_lower_iou_prediction_takes_the_annotation_a_later_better_one_cannot_have():
    m = csr([[(0, 0.4)], [(0, 0.9)]])
    of_pred, iou, matched = EV.match_crowns(m, [1, 1], 0.3, 1)
    assert of_pred.tolist() == [0, -1] and iou.tolist() == [0.4, 0.0] and matched.tolist() == [True]
    of_pred, iou, _ = EV.match_crowns(m, [1, 1], 0.5, 1)                   # the first falls short of the threshold: the second has it
    assert of_pred.tolist() == [-1, 0] and iou.tolist() == [0.0, 0.9]
    # ... and a prediction whose best annotation is taken settles for its next best
    of_pred, iou, matched = EV.match_crowns(csr([[(1, 0.6)], [(0, 0.5), (1, 0.8)]]), [1, 1], 0.3, 2)
    assert of_pred.tolist() == [1, 0] and iou.tolist() == [0.6, 0.5] and matched.tolist() == [True, True]


def test_equal_ious_go_to_the_lowest_annotation_index_in_any_stored_order():
    for row in ([(1, 0.5), (3, 0.5), (4, 0.25)], [(4, 0.25), (3, 0.5), (1, 0.5)]):
        of_pred, _, matched = EV.match_crowns(csr([row]), [1], 0.3, 5)
        assert of_pred.tolist() == [1] and matched.tolist() == [False, True, False, False, False]


def test_iou_equal_to_the_threshold_matches_and_the_next_float_below_does_not():
    for t in (0.3, 0.5, 1.0):
        assert EV.match_crowns(csr([[(0, t)]]), [1], t, 1)[0].tolist() == [0]
        assert EV.match_crowns(csr([[(0, float(np.nextafter(t, 0.0)))]]), [1], t, 1)[0].tolist() == [-1]


def test_an_unselected_prediction_neither_matches_nor_blocks():
    of_pred, iou, matched = EV.match_crowns(csr([[(0, 0.9)], [(0, 0.6)]]), [0, 1], 0.3, 1)
    assert of_pred.tolist() == [-1, 0] and iou.tolist() == [0.0, 0.6] and matched.tolist() == [True]
    assert EV.match_crowns(csr([[(0, 0.9)], [(0, 0.6)]]), [0, 0], 0.3, 1)[2].tolist() == [False]


def test_a_lone_candidate_at_annotation_0_does_match():
    """The reference's ``if not np.any(candidates): continue`` would skip this prediction (its candidate array is [0], which is
    not 'any'); that accident is left out on purpose."""
    of_pred, iou, matched = EV.match_crowns(csr([[(0, 0.8)], []]), [1, 1], 0.3, 2)
    assert of_pred.tolist() == [0, -1] and iou.tolist() == [0.8, 0.0] and matched.tolist() == [True, False]
    assert not np.any(np.array([0]))                                       # the accident itself


def test_zero_iou_entries_never_match_and_empty_sides_are_served():
    assert EV.match_crowns(csr([[(0, 0.0), (1, 0.0)]]), [1], float(np.nextafter(0.0, 1.0)), 2)[0].tolist() == [-1]
    of_pred, iou, matched = EV.match_crowns(csr([]), [], 0.3, 3)
    assert of_pred.shape == (0,) and matched.tolist() == [False] * 3
    of_pred, _, matched = EV.match_crowns(csr([[], []]), [1, 1], 0.3, 0)
    assert of_pred.tolist() == [-1, -1] and matched.shape == (0,)


def test_every_refused_input_returns_invalid():
    lib = _lib.load()
    rs, cl, io = csr([[(0, 0.5), (1, 0.25)], [(1, 0.75)]])
    sel, of_pred, m_iou, matched = np.ones(2, np.uint8), np.zeros(2, np.int32), np.zeros(2), np.zeros(2, np.uint8)
    p = lambda a: a.ctypes.data

    def call(rs=rs, cl=cl, io=io, sel=sel, m=2, n=2, t=0.3, of_pred=of_pred, m_iou=m_iou, matched=matched):
        q = lambda a: None if a is None else p(a)
        return lib.td_match_greedy(q(rs), q(cl), q(io), q(sel), m, n, t, q(of_pred), q(m_iou), q(matched))

    assert call() == 0
    for name in ("rs", "cl", "io", "sel", "of_pred", "m_iou", "matched"):
        assert call(**{name: None}) == _lib.ERR_INVALID and b"null" in lib.td_last_error(), name
    assert call(rs=np.array([0, 3, 2], np.int64)) == _lib.ERR_INVALID and b"decreases" in lib.td_last_error()
    assert call(rs=np.array([1, 2, 3], np.int64)) == _lib.ERR_INVALID
    assert call(cl=np.array([0, 2, 1], np.int32)) == _lib.ERR_INVALID and b"outside" in lib.td_last_error()
    assert call(cl=np.array([0, -1, 1], np.int32)) == _lib.ERR_INVALID
    assert call(io=np.array([0.5, E.NAN, 0.75])) == _lib.ERR_INVALID and b"NaN" in lib.td_last_error()
    for t in (0.0, -0.1, float(np.nextafter(1.0, 2.0)), E.NAN, float("inf")):
        assert call(t=t) == _lib.ERR_INVALID and b"(0, 1]" in lib.td_last_error(), t
    assert call(m=-1) == _lib.ERR_INVALID and call(n=-1) == _lib.ERR_INVALID
    assert call(t=1.0) == 0 and call(t=5e-324) == 0
    with pytest.raises(ValueError, match="NaN"):
        EV.match_crowns((rs, cl, np.array([0.5, E.NAN, 0.75])), [1, 1], 0.3, 2)
    with pytest.raises(ValueError, match="row_start"):
        EV.match_crowns((rs, cl, io), [1, 1, 1], 0.3, 2)


@pytest.mark.parametrize("seed", range(6))
def test_against_the_dense_restatement_of_the_reference_loop(seed):
    """Seeded random sparse matrices; IoUs from a few values so that ties are common; thresholds that equal some of them."""
    rng = np.random.default_rng(1000 + seed)
    m, n = int(rng.integers(1, 60)), int(rng.integers(1, 40))
    values = np.array([0.0, 0.125, 0.25, 0.3, 0.5, 0.625, 0.75, 1.0])
    for density in (0.05, 0.3):
        candidates = rng.uniform(size=(m, n)) < density
        iou = np.where(candidates, rng.choice(values, (m, n)), 0.0)
        matrix = E.csr_of(iou, candidates)
        for t in (0.125, 0.3, 0.5, 0.51, 1.0):
            selected = rng.uniform(size=m) < 0.8
            sub = np.flatnonzero(selected)
            tp, fp, fn, want_of, mean_iou = E.dense_calculate_iou(iou[sub], candidates[sub], t)      # (the reference filters the frame first)
            of_pred, m_iou, matched = EV.match_crowns(matrix, selected, t, n)
            assert np.array_equal(of_pred[sub], want_of) and (of_pred[~selected] == -1).all()
            assert np.array_equal(of_pred[sub] >= 0, tp) and np.array_equal(~matched, fn)
            got = m_iou[of_pred >= 0]
            assert (float(np.mean(got)) if got.size else 0.0) == mean_iou
            assert np.array_equal(m_iou[of_pred >= 0], iou[np.flatnonzero(of_pred >= 0), of_pred[of_pred >= 0]])


# ---- evaluate on the grid of squares ----------------------------------------------------------------------------------------------
def test_grid_ious_keep_their_distance_from_every_threshold():
    """The exact IoUs (rational arithmetic, tests/ring_iou_ref.py) are the fractions the case file names and lie at least 0.05
    from every IoU threshold used; the matrix holds them to a few ulps."""
    pred, _, ann, expect = E.grid_scene()
    row_start, cols, iou = EV.crown_iou_matrix(pred, ann, device=None)
    assert row_start.tolist() == [0, 1, 2, 3, 4, 5, 5] and cols.tolist() == [0, 0, 1, 2, 3]
    for p, want in enumerate(expect):
        for a in range(len(ann)):
            exact = R.exact_iou(pred[p][:-1], ann[a][:-1])
            if want is not None and a == want[0]:
                assert exact == Fraction(int(want[1]), int(want[2]))
                assert all(abs(exact - Fraction(t)) >= Fraction(E.GRID_MARGIN) for t in E.GRID_IOU_THRESHOLDS)
                assert abs(iou[row_start[p]] - float(exact)) <= 1e-12
            else:
                assert exact == 0


def test_evaluate_on_the_grid_gives_the_hand_derived_scores():
    pred, scores, ann, _ = E.grid_scene()
    recs = EV.evaluate(pred, scores, ann, E.GRID_CONFIDENCE_THRESHOLDS, E.GRID_IOU_THRESHOLDS, device=None)
    assert [(r["iou_threshold"], r["confidence_threshold"]) for r in recs] == list(E.GRID_EXPECTED)      # IoU outermost; 0.99 selects nothing: no record
    for r in recs:
        key = (r["iou_threshold"], r["confidence_threshold"])
        tp, fp, fn, tp_list, fn_list = E.GRID_EXPECTED[key]
        assert (r["tp"], r["fp"], r["fn"]) == (tp, fp, fn), key
        assert r["tp_list"].dtype == bool and r["tp_list"].tolist() == tp_list and r["fp_list"].tolist() == [not v for v in tp_list], key
        assert r["fn_list"].dtype == bool and r["fn_list"].tolist() == fn_list, key
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = 2 * precision * recall / (precision + recall) if tp else 0.0
        assert r["precision"] == precision and r["recall"] == recall and r["f1"] == pytest.approx(f1, abs=1e-15), key
        ious = [a / b for a, b in E.GRID_MATCHED_IOUS[key]]
        assert r["mean_iou"] == pytest.approx(float(np.mean(ious)) if ious else 0.0, abs=1e-12), key
        assert set(r) == {"confidence_threshold", "iou_threshold", "precision", "recall", "f1", "mean_iou", "tp", "fp", "fn", "tp_list",
                          "fp_list", "fn_list"}
    first = recs[0]
    assert (first["precision"], first["recall"]) == (0.5, 0.6) and first["f1"] == pytest.approx(6 / 11)


def test_evaluate_without_a_record():
    pred, scores, ann, _ = E.grid_scene()
    assert EV.evaluate(pred, scores, ann, (0.96, 1.5), (0.3, 0.5), device=None) == []               # above every score
    assert EV.evaluate(pred, scores, [], device=None) == []                                         # no annotations
    assert EV.evaluate([], [], ann, device=None) == []
    far = [E.square(E.X0 + 500.0, E.Y0)]                                                            # annotations nobody overlaps: all FP / FN
    (r,) = EV.evaluate(pred, scores, far, (0.3,), (0.3,), device=None)
    assert (r["tp"], r["fp"], r["fn"], r["precision"], r["recall"], r["f1"], r["mean_iou"]) == (0, 6, 1, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="scores"):
        EV.evaluate(pred, scores[:-1], ann, device=None)


# ---- layers ---------------------------------------------------------------------------------------------------------------------
BOW_TIE = np.array([[0.0, 0.0], [10.0, 10.0], [10.0, 0.0], [0.0, 10.0], [0.0, 0.0]]) + np.array([E.X0 + 20.0, E.Y0 + 40.0])


def write_dirs(tmp_path):
    """The grid scene as layers: annotations ``anno_trees_3241.gpkg`` (plus an invalid one and one with Area 0), predictions in a
    sub-folder ``FDOP20_3241_7_rgbi.gpkg`` (plus an invalid one, one that touches the annotations' bounds at a corner only and one a
    hair outside), and files without a partner on either side. The annotations' total bounds: [X0, X0 + 90] x [Y0, Y0 + 10]."""
    pred, scores, ann, _ = E.grid_scene()
    ann_dir, pred_dir = tmp_path / "annotations", tmp_path / "predictions"
    os.makedirs(ann_dir)
    os.makedirs(pred_dir / "combined")
    ann_rings = ann[:2] + [BOW_TIE] + ann[2:] + [E.square(E.X0, E.Y0 + 300.0)]
    gpkg.write_polygons(str(ann_dir / "anno_trees_3241.gpkg"), ann_rings,
                        {"Area": [100.0, 100.0, 50.0, 100.0, 100.0, 100.0, 0.0], "TreeHeight": [12.0, 2.0, 9.0, 14.0, 15.0, 16.0, 17.0]}, 25832)
    gpkg.write_polygons(str(ann_dir / "anno_trees_9999.gpkg"), ann[:1], {"Area": [100.0], "TreeHeight": [10.0]}, 25832)
    corner = E.square(E.X0 + 90.0, E.Y0 + 10.0, 5.0)
    outside = E.square(float(np.nextafter(E.X0 + 90.0, np.inf)), E.Y0 + 10.0, 5.0)
    pred_rings = pred[:3] + [BOW_TIE] + pred[3:] + [corner, outside]
    pred_scores = scores[:3] + [0.99] + scores[3:] + [0.31, 0.32]
    gpkg.write_polygons(str(pred_dir / "combined" / "FDOP20_3241_7_rgbi.gpkg"), pred_rings,
                        {"Confidence_score": pred_scores, "crown_id": list(range(len(pred_rings)))}, 25832)
    gpkg.write_polygons(str(pred_dir / "FDOP20_1234_7_rgbi.gpkg"), pred[:1], {"Confidence_score": [0.5]}, 25832)
    return str(pred_dir), str(ann_dir)


def test_load_drops_invalid_shells_and_filters_by_column(tmp_path):
    pred_dir, ann_dir = write_dirs(tmp_path)
    ann = EV.load_annotations(ann_dir)
    assert sorted(ann) == ["3241", "9999"]
    assert len(ann["3241"]) == 5 and ann["3241"].columns["TreeHeight"] == [12.0, 2.0, 14.0, 15.0, 16.0]          # the bow-tie and Area 0 are gone
    tall = EV.load_annotations(ann_dir, filter_properties=[("Area", 1.0, True), ("TreeHeight", 3.0, True)])
    assert tall["3241"].columns["TreeHeight"] == [12.0, 14.0, 15.0, 16.0] and len(tall["9999"]) == 1
    assert sorted(EV.load_annotations(ann_dir, key=lambda name: name[:4])) == ["anno"]                           # the key function is the caller's
    low = EV.load_annotations(ann_dir, filter_properties=[("Area", 60.0, False)])
    assert low["3241"].columns["Area"] == [0.0]                                                                  # below: the bow-tie (50) is invalid
    with pytest.raises(ValueError, match=r"no column 'MeanNDVI' \(it has \['Area', 'TreeHeight'\]\)"):
        EV.load_annotations(ann_dir, filter_properties=[("MeanNDVI", 0.3, True)])
    pred = EV.load_predictions(pred_dir)
    assert sorted(pred) == ["1234", "3241"]                                                                      # the sub-folder is walked
    assert pred["3241"].columns["crown_id"] == [0, 1, 2, 4, 5, 6, 7, 8]
    assert pred["3241"].blob(3) == gpkg.read_layer(os.path.join(pred_dir, "combined", "FDOP20_3241_7_rgbi.gpkg")).blob(4)


def test_clip_keeps_a_corner_touch_and_drops_a_hair_outside(tmp_path):
    pred_dir, ann_dir = write_dirs(tmp_path)
    said = []
    clipped = EV.clip_predictions(EV.load_predictions(pred_dir), EV.load_annotations(ann_dir), log=said.append)
    assert sorted(clipped) == ["3241"] and said == ["No annotations found for 1234"]
    assert clipped["3241"].columns["crown_id"] == [0, 1, 2, 4, 5, 7]          # 6 lies 100 above the bounds, 8 a hair right of the corner


def test_evaluate_dirs_writes_scores_json_and_matches(tmp_path):
    pred_dir, ann_dir = write_dirs(tmp_path)
    out = str(tmp_path / "out")
    said = []
    results = EV.evaluate_dirs(pred_dir, ann_dir, out, confidence_thresholds=E.GRID_CONFIDENCE_THRESHOLDS, iou_thresholds=E.GRID_IOU_THRESHOLDS,
                               device=None, log=said.append)
    assert list(results) == ["3241"]
    assert "No annotations found for 1234" in said and "No predictions found for 9999" in said
    # the clipped predictions: P0 .. P4 and the corner square (0.31: one more FP at c = 0.3); P5 is clipped away
    lines = open(os.path.join(out, "3241_scores.txt")).read().splitlines()
    assert len(lines) == len(E.GRID_EXPECTED) == len(results["3241"])
    assert lines[0] == "IoU Threshold: 0.3 | Confidence Threshold: 0.3 | Precision: 0.50 | Recall: 0.60 | F1: 0.55 | TP: 3 | FP: 3 | FN: 2 | Mean IoU: 0.698"
    assert lines[3] == "IoU Threshold: 0.3 | Confidence Threshold: 0.95 | Precision: 0.00 | Recall: 0.00 | F1: 0.00 | TP: 0 | FP: 1 | FN: 5 | Mean IoU: 0.000"
    assert lines[8] == "IoU Threshold: 0.75 | Confidence Threshold: 0.3 | Precision: 0.33 | Recall: 0.40 | F1: 0.36 | TP: 2 | FP: 4 | FN: 3 | Mean IoU: 0.909"
    for line, rec in zip(lines, results["3241"]):
        key = (rec["iou_threshold"], rec["confidence_threshold"])
        assert (rec["tp"], rec["fp"], rec["fn"]) == E.GRID_EXPECTED[key][:3] and line == EV.score_line(rec)
    saved = json.load(open(os.path.join(out, "evaluation_results.json")))
    assert list(saved) == ["3241"] and len(saved["3241"]) == len(lines)
    assert saved["3241"][0] == {"confidence_threshold": 0.3, "iou_threshold": 0.3, "precision": 0.5, "recall": 0.6, "f1": results["3241"][0]["f1"],
                                "mean_iou": results["3241"][0]["mean_iou"], "tp": 3, "fp": 3, "fn": 2}
    # the matches layer at (IoU 0.5, confidence 0.3): the selected predictions, then the annotations; blobs untouched
    layer = gpkg.read_layer(os.path.join(out, "3241_matches.gpkg"))
    assert layer.columns["source"] == ["prediction"] * 6 + ["annotation"] * 5
    assert layer.columns["match"] == ["FP", "TP", "TP", "TP", "FP", "FP"] + ["matched", "matched", "matched", "FN", "FN"]
    assert layer.columns["crown_id"] == [0, 1, 2, 4, 5, 7] + [None] * 5 and layer.columns["Confidence_score"][:3] == [0.9, 0.8, 0.6]
    assert layer.columns["match_iou"][:6] == pytest.approx([0.0, 9 / 11, 1.0, 8 / 12, 0.0, 0.0], abs=1e-12) and layer.columns["match_iou"][6:] == [None] * 5
    src_pred = gpkg.read_layer(os.path.join(pred_dir, "combined", "FDOP20_3241_7_rgbi.gpkg"))
    src_ann = gpkg.read_layer(os.path.join(ann_dir, "anno_trees_3241.gpkg"))
    assert layer.blobs == [src_pred.blob(i) for i in (0, 1, 2, 4, 5, 7)] + [src_ann.blob(i) for i in (0, 1, 3, 4, 5)]
    assert layer.srs_id == 25832
    # a second run APPENDS to the score file, as the reference does, and other thresholds write no matches layer
    os.remove(os.path.join(out, "3241_matches.gpkg"))
    EV.evaluate_dirs(pred_dir, ann_dir, out, confidence_thresholds=(0.5,), iou_thresholds=(0.3,), device=None, log=said.append)
    assert len(open(os.path.join(out, "3241_scores.txt")).read().splitlines()) == len(lines) + 1
    assert not os.path.exists(os.path.join(out, "3241_matches.gpkg"))
    with pytest.raises(ValueError, match="no column 'Score'"):
        EV.evaluate_dirs(pred_dir, ann_dir, out, score_field="Score", device=None, log=said.append)


def test_the_command_line_front_pairs_files_by_pattern(tmp_path):
    """tools/evaluate.py on layers named the way the crown stage names them (processed_<name>.gpkg), in this process."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pred, scores, ann, _ = E.grid_scene()
    os.makedirs(tmp_path / "p")
    os.makedirs(tmp_path / "a")
    gpkg.write_polygons(str(tmp_path / "p" / "processed_3241.gpkg"), pred, {"Confidence_score": scores}, 25832)
    gpkg.write_polygons(str(tmp_path / "a" / "3241_annotated.gpkg"), ann, {"Area": [100.0] * 5}, 25832)
    assert tool.main([str(tmp_path / "p"), str(tmp_path / "a"), str(tmp_path / "o"), "--host", "--prediction-pattern", r"processed_(.+)\.gpkg",
                      "--annotation-pattern", r"(.+)_annotated\.gpkg", "--iou", "0.5", "--confidence", "0.3", "0.5"]) == 0
    assert sorted(os.listdir(tmp_path / "o")) == ["3241_matches.gpkg", "3241_scores.txt", "evaluation_results.json"]
    assert open(tmp_path / "o" / "3241_scores.txt").read().splitlines()[0].startswith("IoU Threshold: 0.5 | Confidence Threshold: 0.3 | Precision: 0.60")
