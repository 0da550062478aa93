"""Scoring predicted crowns against annotated crowns (reference supplementary/evaluation_compute_scores.py: ``load_annotations``,
``load_predictions``, ``clip_predictions``, ``calculate_iou``, ``evaluate`` and the loop of its ``main``): IoU-matched precision /
recall / F1 / mean IoU per confidence threshold and per IoU threshold, and the TP / FP / FN lists per crown.

What runs where: the candidate pairs between the two sets come from their float64 boxes (box_pairs.box_pairs_ab) — ``td_box_pairs_ab_count`` /
``td_box_pairs_ab_fill`` (boxpairs_ab.hip), or with ``device=None`` the host twin ``td_box_pairs_ab``, the same set for any input;
the intersection area of every candidate pair is one launch of ``td_ring_pairs_area_dev`` (or its host twin, same bits:
cleaning.ring_pairs_area_packed); IoU is formed in cleaning.iou_of and nowhere else. That sparse IoU matrix of an image is
computed ONCE; every (confidence threshold, IoU threshold) combination is then one linear pass of ``td_match_greedy`` over it,
where the reference recomputes every shapely overlay for each combination.

The matching rule is the reference's: predictions in the FILE's order (not by score), each takes the still unmatched annotation
with the largest IoU — the lowest annotation index among equals, as ``np.argmax`` keeps the first — when that IoU is
``>= iou_threshold``.

Not reproduced:
  * GEOS' overlay noise in the areas. The areas carry the ring-pair kernel's documented error; a decision whose
    IoU lies within that error of a threshold is unspecified.
  * shapely's ``union().area``: the union here is ``area_a + area_b - inter`` (cleaning.iou_of).
  * Holes and further parts: the shell of a feature's first part is used, as everywhere in this package.
  * The reference's ``if not np.any(candidates): continue``, which tests an array of annotation POSITIONS for truth and so skips a
    prediction whose only candidate is the annotation at position 0 — an accident, deliberately left out: such a prediction
    matches here (tests/test_evaluation.py pins it).
"""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import cleaning as CL
from .box_pairs import box_pairs_ab
from .crown_device import pack_rings, packed_boxes, ring_boxes  # noqa: F401  (ring_boxes: re-exported)

DEFAULT_CONFIDENCE_THRESHOLDS = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
DEFAULT_FILTER_PROPERTIES = (("Area", 0.0, True),)
SCORE_FIELD = "Confidence_score"

Matrix = Tuple[np.ndarray, np.ndarray, np.ndarray]      # row_start int64 [m + 1], cols int32, iou float64


# ---- the sparse IoU matrix of an image ----------------------------------------------------------------------------------------
def crown_iou_matrix(pred_rings: Sequence, ann_rings: Sequence, device: Optional[int] = 0) -> Matrix:
    """The IoU of every prediction with every annotation it overlaps, as CSR rows over the predictions → (row_start int64 [m + 1],
    cols int32 = annotation indices, ascending within a row, iou float64): :func:`box_pairs_ab` on the rings' boxes,
    cleaning.ring_pairs_area_packed on the candidates (pairs over the kernel's vertex cap go to the host function there, same bits),
    cleaning.iou_of; only entries with ``iou > 0`` are kept. Rings: [k, 2] vertex arrays, closed or open, simple, either winding.
    ``device``: a GPU index, or None for the host functions — the same matrix bit for bit. ValueError for a candidate pair the
    area function refuses (a ring of fewer than 3 vertices, a non-finite coordinate)."""
    m = len(pred_rings)
    xy_a, start_a = pack_rings(pred_rings)
    xy_b, start_b = pack_rings(ann_rings)
    pairs = box_pairs_ab(packed_boxes(xy_a, start_a), packed_boxes(xy_b, start_b), device)
    if pairs.shape[0] == 0:
        return np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)
    areas, status = CL.ring_pairs_area_packed(xy_a, start_a, xy_b, start_b, pairs, device)
    bad = np.flatnonzero((status == 2) | np.isnan(areas[:, 0]))
    if bad.size:
        i, j = pairs[bad[0]]
        raise ValueError(f"crown_iou_matrix: prediction {int(i)} / annotation {int(j)} is refused: a ring of fewer than 3 vertices or a "
                         f"non-finite coordinate ({bad.size} such pairs)")
    iou = CL.iou_of(areas)
    keep = iou > 0
    pairs, iou = pairs[keep], iou[keep]
    row_start = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=m), out=row_start[1:])
    return row_start, np.ascontiguousarray(pairs[:, 1], dtype=np.int32), np.ascontiguousarray(iou, dtype=np.float64)


# ---- the matching ---------------------------------------------------------------------------------------------------------------
def match_crowns(matrix: Matrix, selected, iou_threshold: float, n_ann: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """td_match_greedy: the reference's ``calculate_iou`` loop over the sparse matrix → (match_of_pred int32 [m]: the annotation
    index or -1, match_iou float64 [m], ann_matched bool [n_ann]). ``selected``: bool [m], the predictions that take part (the
    others neither match nor block). ValueError for what the library refuses: a malformed matrix, a NaN IoU, a threshold outside
    (0, 1]."""
    rs = np.ascontiguousarray(matrix[0], dtype=np.int64)
    cl = np.ascontiguousarray(matrix[1], dtype=np.int32)
    io = np.ascontiguousarray(matrix[2], dtype=np.float64)
    sel = np.ascontiguousarray(selected, dtype=np.uint8)
    m = sel.shape[0]
    if sel.ndim != 1 or rs.shape != (m + 1,) or cl.ndim != 1 or io.shape != cl.shape or (rs.size and cl.shape[0] != int(rs[-1])):
        raise ValueError("match_crowns: row_start needs m + 1 entries for m = len(selected), cols and iou row_start[m] each")
    of_pred, m_iou, matched = np.full(m, -1, np.int32), np.zeros(m), np.zeros(max(int(n_ann), 0), np.uint8)
    st = _lib.load().td_match_greedy(rs.ctypes.data, cl.ctypes.data, io.ctypes.data, sel.ctypes.data, m, int(n_ann), float(iou_threshold),
                                     of_pred.ctypes.data, m_iou.ctypes.data, matched.ctypes.data)
    if st == _lib.ERR_INVALID:
        raise ValueError(f"match_crowns: {_lib.load().td_last_error().decode('utf-8', 'replace')}")
    _lib.check(st, "td_match_greedy")
    return of_pred, m_iou, matched.astype(bool)


def _score(matrix: Matrix, scores: np.ndarray, n_ann: int, confidence_threshold: float, iou_threshold: float) -> Optional[dict]:
    """One (confidence, IoU) combination on the matrix → its record (with ``selected`` and ``match_iou`` besides the public fields),
    or None when no prediction reaches the confidence threshold."""
    with np.errstate(invalid="ignore"):
        selected = scores >= confidence_threshold
    if not selected.any():
        return None
    of_pred, m_iou, ann_matched = match_crowns(matrix, selected, iou_threshold, n_ann)
    tp_list = of_pred[selected] >= 0
    fp_list = ~tp_list
    fn_list = ~ann_matched
    tp, fp, fn = int(tp_list.sum()), int(fp_list.sum()), int(fn_list.sum())
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0
    f1 = 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0
    matched_iou = m_iou[of_pred >= 0]
    return {"confidence_threshold": confidence_threshold, "iou_threshold": iou_threshold, "precision": float(precision),
            "recall": float(recall), "f1": float(f1), "mean_iou": float(np.mean(matched_iou)) if matched_iou.size else 0.0,
            "tp": tp, "fp": fp, "fn": fn, "tp_list": tp_list, "fp_list": fp_list, "fn_list": fn_list,
            "selected": np.flatnonzero(selected), "match_iou": m_iou[selected]}


_PRIVATE = ("selected", "match_iou")


def _scores_array(scores, m: int) -> np.ndarray:
    s = np.array([np.nan if v is None else float(v) for v in scores], dtype=np.float64)
    if s.shape != (m,):
        raise ValueError(f"evaluate: {m} prediction rings but {s.size} scores")
    return s


def evaluate(pred_rings: Sequence, scores: Sequence, ann_rings: Sequence,
             confidence_thresholds: Sequence[float] = DEFAULT_CONFIDENCE_THRESHOLDS, iou_thresholds: Sequence[float] = (0.3,),
             device: Optional[int] = 0) -> List[dict]:
    """The reference's ``evaluate`` for one image → one record per (IoU threshold, confidence threshold), IoU thresholds outermost:
    ``confidence_threshold``, ``iou_threshold``, ``precision``, ``recall``, ``f1``, ``mean_iou``, ``tp``, ``fp``, ``fn`` and the bool
    arrays ``tp_list`` / ``fp_list`` (over the predictions with ``score >= confidence_threshold``, in order) and ``fn_list`` (over
    the annotations). precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 p r / (p + r), each 0 on a zero denominator;
    ``mean_iou`` = np.mean of the matched IoUs in matching order, 0.0 when nothing matched. A confidence threshold no score reaches
    yields no record; no predictions or no annotations yield no records. The IoU matrix is computed once (:func:`crown_iou_matrix`
    on ``device``, None = host; same records bit for bit)."""
    s = _scores_array(scores, len(pred_rings))
    if len(pred_rings) == 0 or len(ann_rings) == 0:
        return []
    matrix = crown_iou_matrix(pred_rings, ann_rings, device)
    out = []
    for t in iou_thresholds:
        for c in confidence_thresholds:
            rec = _score(matrix, s, len(ann_rings), c, t)
            if rec is not None:
                out.append({k: v for k, v in rec.items() if k not in _PRIVATE})
    return out


# ---- layers ---------------------------------------------------------------------------------------------------------------------
def annotation_key(filename: str) -> str:
    """The reference's identifier of an annotation file: ``anno_<category>_<id>.gpkg`` → ``<id>``."""
    return filename.split('_')[2].split('.')[0]


def prediction_key(filename: str) -> str:
    """The reference's identifier of a prediction file: ``FDOP20_<id>_..._.gpkg`` → ``<id>``."""
    return filename.split('_')[1]


def _valid_subset(layer, keep_extra: Optional[np.ndarray] = None):
    """The features of a Layer whose shell is non-empty and valid (td_ring_is_valid: GEOS' rules), as a Layer."""
    from .gpkg import Layer
    from .validity import ring_is_valid

    keep = []
    for i, r in enumerate(layer.rings()):
        r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
        if r.shape[0] >= 4 and (keep_extra is None or keep_extra[i]) and ring_is_valid(r):
            keep.append(i)
    return Layer([layer.blob(i) for i in keep], {n: [v[i] for i in keep] for n, v in layer.columns.items()}, layer.srs_id)


def _gpkg_files(folder: str, walk: bool) -> List[str]:
    if walk:
        return sorted(os.path.join(root, f) for root, _, files in os.walk(folder) for f in files if f.endswith(".gpkg"))
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(".gpkg"))


def _load(folder: str, key: Callable[[str], str], walk: bool, filter_properties, who: str, log) -> Dict[str, object]:
    from .gpkg import read_layer

    out = {}
    for path in _gpkg_files(folder, walk):
        name = os.path.basename(path)
        try:
            identifier = key(name)
        except IndexError:
            log(f"{who}: {name} does not follow the naming pattern: skipped")
            continue
        layer = read_layer(path)
        if len(layer) == 0:
            continue
        keep = np.ones(len(layer), bool)
        for column, threshold, above in filter_properties:
            if column not in layer.columns:
                raise ValueError(f"{who}: {path} has no column {column!r} (it has {sorted(layer.columns)})")
            v = np.array([np.nan if x is None else float(x) for x in layer.columns[column]], dtype=np.float64)
            with np.errstate(invalid="ignore"):
                keep &= (v > threshold) if above else (v < threshold)
        out[identifier] = _valid_subset(layer, keep)
    return out


def load_annotations(annotation_dir: str, filter_properties=DEFAULT_FILTER_PROPERTIES, key: Callable[[str], str] = annotation_key,
                     log=print) -> Dict[str, object]:
    """identifier → gpkg.Layer of the ``.gpkg`` files of ``annotation_dir``: features with an empty or invalid shell dropped, then
    those that fail a filter — ``filter_properties``: (column, threshold, above) keeps ``column > threshold`` (``above``) or
    ``column < threshold``; a missing value fails. Empty files are left out. ValueError for a column a file lacks."""
    return _load(annotation_dir, key, False, tuple(filter_properties), "load_annotations", log)


def load_predictions(prediction_dir: str, key: Callable[[str], str] = prediction_key, log=print) -> Dict[str, object]:
    """identifier → gpkg.Layer of every ``.gpkg`` file under ``prediction_dir`` (walked), invalid and empty shells dropped."""
    return _load(prediction_dir, key, True, (), "load_predictions", log)


def _total_bounds(rings: Sequence[np.ndarray]) -> Tuple[float, float, float, float]:
    xy = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings])
    return float(xy[:, 0].min()), float(xy[:, 1].min()), float(xy[:, 0].max()), float(xy[:, 1].max())


def clip_predictions(predictions: Dict[str, object], annotations: Dict[str, object], log=print) -> Dict[str, object]:
    """Per identifier the predictions whose polygon ``intersects`` the closed box of the annotations' total bounds — decided
    exactly by td_region_relate (csrc/geom_predicates.h): touching the box in one point counts, as in GEOS. Identifiers without
    annotations are logged and left out, as are pairs with an empty side."""
    from .gpkg import Layer
    from .vector import Region, box_ring

    out = {}
    for identifier, pred in predictions.items():
        if identifier not in annotations:
            log(f"No annotations found for {identifier}")
            continue
        ann = annotations[identifier]
        if len(ann) == 0 or len(pred) == 0:
            continue
        hit, _ = Region([[box_ring(*_total_bounds(ann.rings()))]]).relate(pred.rings())
        keep = np.flatnonzero(hit)
        out[identifier] = Layer([pred.blob(i) for i in keep], {n: [v[i] for i in keep] for n, v in pred.columns.items()}, pred.srs_id)
    return out


def score_line(rec: dict) -> str:
    """One line of ``<id>_scores.txt`` in the reference's format."""
    return (f"IoU Threshold: {rec['iou_threshold']} | Confidence Threshold: {rec['confidence_threshold']} | "
            f"Precision: {rec['precision']:.2f} | Recall: {rec['recall']:.2f} | F1: {rec['f1']:.2f} | "
            f"TP: {rec['tp']} | FP: {rec['fp']} | FN: {rec['fn']} | Mean IoU: {rec['mean_iou']:.3f}")


def _write_matches(path: str, pred, ann, rec: dict) -> None:
    """``<id>_matches.gpkg``: one layer — the predictions the record selected with their columns, ``match`` = TP / FP and
    ``match_iou``; then the annotations with ``match`` = matched / FN; ``source`` tells the two apart. Blobs untouched."""
    from .gpkg import write_blobs

    sel = [int(i) for i in rec["selected"]]
    n_p, n_a = len(sel), len(ann)
    cols = {"source": ["prediction"] * n_p + ["annotation"] * n_a,
            "match": ["TP" if v else "FP" for v in rec["tp_list"]] + ["FN" if v else "matched" for v in rec["fn_list"]],
            "match_iou": [float(v) for v in rec["match_iou"]] + [None] * n_a}
    for name, values in pred.columns.items():
        cols[name if name not in cols else name + "_"] = [values[i] for i in sel] + [None] * n_a
    blobs = [pred.blob(i) for i in sel] + [ann.blob(j) for j in range(n_a)]
    write_blobs(path, blobs, cols, pred.srs_id, _total_bounds([pred.rings()[i] for i in sel] + ann.rings()))


def evaluate_dirs(prediction_dir: str, annotation_dir: str, out_dir: str,
                  confidence_thresholds: Sequence[float] = DEFAULT_CONFIDENCE_THRESHOLDS,
                  iou_thresholds: Sequence[float] = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9),
                  filter_properties=DEFAULT_FILTER_PROPERTIES, score_field: str = SCORE_FIELD,
                  matches_iou_threshold: float = 0.5, matches_confidence_threshold: float = 0.3,
                  annotation_key: Callable[[str], str] = annotation_key, prediction_key: Callable[[str], str] = prediction_key,
                  device: Optional[int] = 0, log=print) -> Dict[str, List[dict]]:
    """The loop of the reference's ``main`` for one prediction folder: load both folders, pair the files by identifier (both key
    functions overridable; identifiers without a partner are logged), clip the predictions to the annotations' bounds, and per
    identifier compute the IoU matrix once and score every (IoU threshold, confidence threshold). Written to ``out_dir``:
    ``<id>_scores.txt`` (one line per record APPENDED, the reference's format), ``evaluation_results.json`` (identifier → the
    records without their per-crown lists) and, in place of the reference's picture, ``<id>_matches.gpkg`` at
    (``matches_iou_threshold``, ``matches_confidence_threshold``) when both are among the thresholds and a prediction is selected
    there. → identifier → records (as :func:`evaluate` returns them). ValueError when a prediction file lacks ``score_field``."""
    os.makedirs(out_dir, exist_ok=True)
    annotations = load_annotations(annotation_dir, filter_properties, annotation_key, log)
    predictions = load_predictions(prediction_dir, prediction_key, log)
    for identifier in annotations:
        if identifier not in predictions:
            log(f"No predictions found for {identifier}")
    clipped = clip_predictions(predictions, annotations, log)
    results: Dict[str, List[dict]] = {}
    for identifier, ann in annotations.items():
        pred = clipped.get(identifier)
        if pred is None or len(pred) == 0 or len(ann) == 0:
            continue
        if score_field not in pred.columns:
            raise ValueError(f"evaluate_dirs: the predictions of {identifier} have no column {score_field!r} (they have {sorted(pred.columns)})")
        scores = _scores_array(pred.columns[score_field], len(pred))
        matrix = crown_iou_matrix(pred.rings(), ann.rings(), device)
        for t in iou_thresholds:
            for c in confidence_thresholds:
                rec = _score(matrix, scores, len(ann), c, t)
                if rec is None:
                    continue
                line = score_line(rec)
                with open(os.path.join(out_dir, f"{identifier}_scores.txt"), "a") as f:
                    f.write(line + "\n")
                log(line)
                if t == matches_iou_threshold and c == matches_confidence_threshold:
                    _write_matches(os.path.join(out_dir, f"{identifier}_matches.gpkg"), pred, ann, rec)
                results.setdefault(identifier, []).append({k: v for k, v in rec.items() if k not in _PRIVATE})
    summary = {identifier: [{k: v for k, v in rec.items() if not isinstance(v, np.ndarray)} for rec in recs] for identifier, recs in results.items()}
    with open(os.path.join(out_dir, "evaluation_results.json"), "w") as f:
        json.dump(summary, f, indent=4)
    log(f"Saved JSON results to {os.path.join(out_dir, 'evaluation_results.json')}")
    return results
