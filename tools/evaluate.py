"""Score predicted crown layers against annotated ones (treedetection_amd.evaluation.evaluate_dirs; the reference's
supplementary/evaluation_compute_scores.py for one prediction folder).

    python tools/evaluate.py <prediction_dir> <annotation_dir> <out_dir> [--device 0 | --host] [--iou 0.3 0.5 ...] [--confidence 0.3 ...]
        [--filter Area 0.0 above ...] [--prediction-pattern REGEX] [--annotation-pattern REGEX]

Files are paired by identifier: by default the reference's rule (annotation ``anno_<category>_<id>.gpkg``, prediction
``FDOP20_<id>_...gpkg``); ``--prediction-pattern`` / ``--annotation-pattern`` take a regular expression whose first group is the
identifier instead, e.g. ``--prediction-pattern 'processed_(.+)\\.gpkg'`` for the layers the crown stage writes. Writes
``<id>_scores.txt``, ``<id>_matches.gpkg`` and ``evaluation_results.json`` into ``out_dir``."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pattern_key(pattern):
    rx = re.compile(pattern)

    def key(name):
        m = rx.search(name)
        if m is None or not m.groups():
            raise IndexError(name)          # (what the default keys raise for a name outside their pattern: logged and skipped)
        return m.group(1)

    return key


def main(argv=None):
    from treedetection_amd import evaluation as EV

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("prediction_dir")
    ap.add_argument("annotation_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--device", type=int, default=0, help="GPU index (default 0)")
    ap.add_argument("--host", action="store_true", help="the host functions instead of the GPU (same results)")
    ap.add_argument("--iou", type=float, nargs="+", default=[0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9])
    ap.add_argument("--confidence", type=float, nargs="+", default=list(EV.DEFAULT_CONFIDENCE_THRESHOLDS))
    ap.add_argument("--filter", nargs=3, action="append", metavar=("COLUMN", "THRESHOLD", "above|below"),
                    help="keep annotations with COLUMN above / below THRESHOLD (default: Area 0.0 above); may repeat")
    ap.add_argument("--no-filter", action="store_true", help="no annotation filter at all")
    ap.add_argument("--score-field", default=EV.SCORE_FIELD)
    ap.add_argument("--matches-iou", type=float, default=0.5)
    ap.add_argument("--matches-confidence", type=float, default=0.3)
    ap.add_argument("--prediction-pattern")
    ap.add_argument("--annotation-pattern")
    args = ap.parse_args(argv)
    filters = EV.DEFAULT_FILTER_PROPERTIES
    if args.no_filter:
        filters = ()
    elif args.filter:
        for _, _, how in args.filter:
            if how not in ("above", "below"):
                ap.error(f"--filter: {how!r} is neither above nor below")
        filters = tuple((c, float(t), how == "above") for c, t, how in args.filter)
    results = EV.evaluate_dirs(args.prediction_dir, args.annotation_dir, args.out_dir, confidence_thresholds=args.confidence,
                               iou_thresholds=args.iou, filter_properties=filters, score_field=args.score_field,
                               matches_iou_threshold=args.matches_iou, matches_confidence_threshold=args.matches_confidence,
                               annotation_key=pattern_key(args.annotation_pattern) if args.annotation_pattern else EV.annotation_key,
                               prediction_key=pattern_key(args.prediction_pattern) if args.prediction_pattern else EV.prediction_key,
                               device=None if args.host else args.device)
    print(f"{len(results)} image(s) scored")
    return 0


if __name__ == "__main__":
    sys.exit(main())
