"""clean_crowns by polygon IoU at the size the crown stage is built for: a synthetic layer of 20 000 star-shaped crowns of 20 - 60
vertices (radius 1.5 - 6 m, lobed outlines) on a jittered grid at UTM coordinates with the overlap of a closed canopy, every
tenth followed by a shrunk near-duplicate; seeded.

    python tools/clean_crowns_bench.py [--n 20000] [--reps 7] [--out profiles/clean_crowns.txt]

Reports: candidate pairs (device kernels and host sweep); pairs the kernel leaves to the host (status 1); the time of the area
launch alone (HIP events around td_ring_pairs_area_dev, after a warm-up launch, median of --reps); the same pairs through the host
function td_ring_pairs_area (one thread, wall clock); the wall time of clean_crowns(device=0) against clean_crowns(device=None)
in this process (median of 3 after one warm-up each), and whether the two kept lists and the two area arrays are identical.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n, seed=0):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    pitch = 7.0                                              # 20 000 crowns: 990 m x 990 m
    rings, k = [], 0
    while len(rings) < n:
        c = np.array([412010.0 + pitch * (k % side), 5318010.0 + pitch * (k // side)]) + rng.uniform(-2.5, 2.5, 2)
        m = int(rng.integers(20, 61))
        ang = (np.arange(m) + rng.uniform(0.2, 0.8, m)) * (2 * np.pi / m)
        r = rng.uniform(1.5, 6.0) * (1 + 0.15 * np.sin(rng.integers(2, 6) * ang + rng.uniform(0, 6)) + rng.uniform(-0.05, 0.05, m))
        ring = np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], axis=1)
        rings.append(np.concatenate([ring, ring[:1]]))
        if k % 10 == 9:
            dup = c + (ring - c) * rng.uniform(0.88, 0.98) + rng.uniform(-0.1, 0.1, 2)
            rings.append(np.concatenate([dup, dup[:1]]))
        k += 1
    return rings[:n], [float(v) for v in rng.uniform(0.3, 1.0, n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from treedetection_amd import _lib
    from treedetection_amd import cleaning as CL

    if not torch.cuda.is_available():
        raise SystemExit("clean_crowns_bench needs a GPU")
    rings, scores = scene(args.n)
    opened = [CL.open_ring(r) for r in rings]
    boxes = np.array([[o[:, 0].min(), o[:, 1].min(), o[:, 0].max(), o[:, 1].max()] for o in opened])
    res = {"n": args.n, "vertices": int(sum(len(o) for o in opened)), "device": torch.cuda.get_device_name(0)}

    CL.candidate_pairs(boxes[:64], 0)                        # the context, the library and torch's allocator exist
    t = time.perf_counter()
    pairs = CL.candidate_pairs(boxes, 0)
    res["candidate_pairs_device_wall_ms"] = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    host_pairs = CL.candidate_pairs_host(boxes)
    res["candidate_pairs_host_wall_ms"] = 1e3 * (time.perf_counter() - t)
    res["candidate_pairs"], res["candidate_pairs_host"] = int(len(pairs)), int(len(host_pairs))
    res["device_pairs_cover_host_pairs"] = bool({tuple(p) for p in host_pairs.tolist()} <= {tuple(p) for p in pairs.tolist()})

    xy, start = CL.pack_rings(opened)
    terms = (np.diff(start)[pairs[:, 0]] * np.diff(start)[pairs[:, 1]]).astype(np.int64)
    res["terms"] = int(terms.sum())
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    d_xy, d_start, d_pairs = (torch.from_numpy(a).to(dev) for a in (xy, start, pairs))
    d_out = torch.empty((len(pairs), 3), dtype=torch.float64, device=dev)
    d_status = torch.empty(len(pairs), dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.td_ring_pairs_area_dev(d_xy.data_ptr(), d_start.data_ptr(), len(opened), d_xy.data_ptr(), d_start.data_ptr(), len(opened),
                                              d_pairs.data_ptr(), len(pairs), d_out.data_ptr(), d_status.data_ptr(), _lib.stream_ptr()),
                   "td_ring_pairs_area_dev")

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
    res["area_launch_ms"] = {"median": statistics.median(times), "min": min(times), "max": max(times)}
    res["area_launch_terms_per_s"] = res["terms"] / (1e-3 * statistics.median(times))
    status = d_status.cpu().numpy()
    res["pairs_status_1"], res["pairs_status_2"] = int((status == 1).sum()), int((status == 2).sum())

    times = []
    for _ in range(3):
        t = time.perf_counter()
        h_out, h_status = CL.ring_pairs_area_packed(xy, start, xy, start, pairs, None)
        times.append(1e3 * (time.perf_counter() - t))
    res["area_host_function_wall_ms"] = {"median": statistics.median(times), "min": min(times), "max": max(times)}
    res["areas_identical"] = bool(np.array_equal(d_out.cpu().numpy().view(np.uint64), h_out.view(np.uint64)) and (h_status == status).all())

    kept = {}
    for name, device in (("device", 0), ("host", None), ("device", 0), ("host", None)):       # alternated; the first of each warms up
        runs = []
        for _ in range(2):
            t = time.perf_counter()
            kept[name] = CL.clean_crowns(rings, scores, device=device)
            runs.append(1e3 * (time.perf_counter() - t))
        res.setdefault(f"clean_crowns_{name}_wall_ms", []).extend(runs)
    for name in ("device", "host"):
        runs = res[f"clean_crowns_{name}_wall_ms"][1:]
        res[f"clean_crowns_{name}_wall_ms"] = {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}
    res["kept"], res["kept_lists_identical"] = len(kept["device"]), kept["device"] == kept["host"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# python tools/clean_crowns_bench.py --n {args.n} --reps {args.reps}\n{text}\n")


if __name__ == "__main__":
    main()
