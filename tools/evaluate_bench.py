"""The evaluation stage at the size the crown stage is built for: the 20 000 seeded crowns of tools/clean_crowns_bench.py as
predictions against about 15 000 shifted and rescaled copies of them as annotations.

    python tools/evaluate_bench.py [--n 20000] [--reps 10] [--out profiles/evaluation.txt]

Reports: HIP events around td_box_pairs_ab_count, td_box_pairs_ab_fill and td_ring_pairs_area_dev (mean of --reps after a warm-up
launch each); the wall time of box_pairs_ab on the device and of the host twin; of the parent's only alternatives on the two box
sets concatenated — cleaning.candidate_pairs_host and cleaning.candidate_pairs, the pairs within one set discarded afterwards —;
of crown_iou_matrix; and of the full 7 x 7 evaluate at device=0 and device=None (median of 3 after one warm-up each), and whether
all of them agree. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def annotations_of(rings, seed=1, keep=0.75):
    rng = np.random.default_rng(seed)
    out = []
    for ring in rings:
        if rng.uniform() < keep:
            o = ring[:-1]
            c = o.mean(axis=0)
            moved = c + (o - c) * rng.uniform(0.8, 1.15) + rng.uniform(-0.6, 0.6, 2)
            out.append(np.concatenate([moved, moved[:1]]))
    return out


def wall(fn, reps=3):
    fn()
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        result = fn()
        runs.append(1e3 * (time.perf_counter() - t))
    return {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from clean_crowns_bench import scene
    from treedetection_amd import _lib
    from treedetection_amd import cleaning as CL
    from treedetection_amd import evaluation as EV

    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench needs a GPU")
    pred, scores = scene(args.n)
    ann = annotations_of(pred)
    pa, pb = [CL.open_ring(r) for r in pred], [CL.open_ring(r) for r in ann]
    boxes_a, boxes_b = EV.ring_boxes(pa), EV.ring_boxes(pb)
    n_a, n_b = len(pa), len(pb)
    res = {"predictions": n_a, "annotations": n_b, "device": torch.cuda.get_device_name(0)}
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    EV.box_pairs_ab(boxes_a[:64], boxes_b[:64], 0)             # the context, the library and torch's allocator exist

    # ---- the launches alone, HIP events
    d_a, d_b = torch.from_numpy(boxes_a).to(dev), torch.from_numpy(boxes_b).to(dev)
    counts = torch.empty(n_a, dtype=torch.int32, device=dev)
    count = lambda: _lib.check(lib.td_box_pairs_ab_count(d_a.data_ptr(), n_a, d_b.data_ptr(), n_b, counts.data_ptr(), _lib.stream_ptr()), "count")
    count()
    row_start = torch.zeros(n_a + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=row_start[1:])
    total = int(row_start[-1].item())
    cols = torch.empty(total, dtype=torch.int32, device=dev)
    cursor = torch.empty(n_a, dtype=torch.int32, device=dev)
    fill = lambda: _lib.check(lib.td_box_pairs_ab_fill(d_a.data_ptr(), n_a, d_b.data_ptr(), n_b, row_start.data_ptr(), cursor.data_ptr(),
                                                       cols.data_ptr(), _lib.stream_ptr()), "fill")
    pairs = EV.box_pairs_ab(boxes_a, boxes_b, 0)
    xy_a, start_a = CL.pack_rings(pa)
    xy_b, start_b = CL.pack_rings(pb)
    d_xa, d_sa, d_xb, d_sb, d_p = (torch.from_numpy(v).to(dev) for v in (xy_a, start_a, xy_b, start_b, pairs))
    d_out = torch.empty((len(pairs), 3), dtype=torch.float64, device=dev)
    d_status = torch.empty(len(pairs), dtype=torch.int32, device=dev)
    area = lambda: _lib.check(lib.td_ring_pairs_area_dev(d_xa.data_ptr(), d_sa.data_ptr(), n_a, d_xb.data_ptr(), d_sb.data_ptr(), n_b, d_p.data_ptr(),
                                                         len(pairs), d_out.data_ptr(), d_status.data_ptr(), _lib.stream_ptr()), "area")

    def events(launch):
        launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return {"mean": statistics.mean(times), "min": min(times), "max": max(times)}

    res["candidate_pairs"] = int(len(pairs))
    res["pair_tests"] = n_a * n_b
    res["count_launch_ms"] = events(count)
    res["fill_launch_ms"] = events(fill)
    res["area_launch_ms"] = events(area)
    res["area_terms"] = int((np.diff(start_a)[pairs[:, 0]] * np.diff(start_b)[pairs[:, 1]]).astype(np.int64).sum())

    # ---- wall times
    res["box_pairs_ab_device_wall_ms"], dev_pairs = wall(lambda: EV.box_pairs_ab(boxes_a, boxes_b, 0))
    res["box_pairs_ab_host_wall_ms"], host_pairs = wall(lambda: EV.box_pairs_ab(boxes_a, boxes_b, None))
    res["device_pairs_equal_host_pairs"] = bool(np.array_equal(dev_pairs, host_pairs))
    both = np.concatenate([boxes_a, boxes_b])

    def across(p):                                                  # the pairs of one concatenated set that join A with B
        p = p[(p[:, 0] < n_a) & (p[:, 1] >= n_a)]
        return np.stack([p[:, 0], p[:, 1] - n_a], axis=1)

    res["concatenated_candidate_pairs_host_wall_ms"], cat_host = wall(lambda: CL.candidate_pairs_host(both), reps=1)
    res["concatenated_candidate_pairs_device_wall_ms"], cat_dev = wall(lambda: CL.candidate_pairs(both, 0))
    res["concatenated_pairs_all"], res["concatenated_pairs_across"] = int(len(cat_dev)), int(len(across(cat_dev)))
    res["concatenated_host_across_equal"] = bool(np.array_equal(across(cat_host), host_pairs))
    res["concatenated_device_across_cover"] = bool({tuple(p) for p in host_pairs.tolist()} <= {tuple(p) for p in across(cat_dev).tolist()})
    res["crown_iou_matrix_device_wall_ms"], matrix = wall(lambda: EV.crown_iou_matrix(pred, ann, 0))
    res["matrix_entries"] = int(len(matrix[1]))
    thresholds = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
    res["evaluate_7x7_device_wall_ms"], recs_dev = wall(lambda: EV.evaluate(pred, scores, ann, thresholds, thresholds, device=0))
    res["evaluate_7x7_host_wall_ms"], recs_host = wall(lambda: EV.evaluate(pred, scores, ann, thresholds, thresholds, device=None), reps=1)
    t = time.perf_counter()
    for tt in thresholds:
        for c in thresholds:
            EV.match_crowns(matrix, np.asarray(scores) >= c, tt, n_b)
    res["match_49_passes_wall_ms"] = 1e3 * (time.perf_counter() - t)
    same = len(recs_dev) == len(recs_host) and all(
        all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a) for a, b in zip(recs_dev, recs_host))
    res["records"], res["records_identical"] = len(recs_dev), bool(same)
    first = recs_dev[0]
    res["first_record"] = {k: v for k, v in first.items() if not isinstance(v, np.ndarray)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# python tools/evaluate_bench.py --n {args.n} --reps {args.reps}\n{text}\n")


if __name__ == "__main__":
    main()
