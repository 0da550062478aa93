"""Crowns against a forest outline, host and device, at the size the fusion step sees: the 20 000 star-shaped crowns of
tools/clean_crowns_bench.py (UTM coordinates, 990 m x 990 m) against an outline of adjacent parcels — the cells of a jittered
16 x 16 grid taken in 2 x 2 blocks like a chess board, so about half of the area is forest, neighbours share their (jagged)
borders exactly and many crowns straddle one — plus a few clearings (holes) and islands; the borders are subdivided until the
outline has about 10^4, 10^5 and 10^6 vertices. Seeded.

    python tools/region_relate_bench.py [--n 20000] [--sizes 10000 100000 1000000] [--reps 7] [--out profiles/region_relate.txt]

Per outline size, each path in a process of its own (started here, one after the other): the wall time of Region.relate on the
host (td_region_relate, one thread; its own index build included), the wall time of Region.relate(device=0) on a fresh Region
(index build, packing, upload, launch, copy back and the deferred host work included) and on the same Region again (the second
layer of a fusion: region and index already uploaded), the launch alone (HIP events around td_region_relate_dev, median of --reps),
the queries the kernel left to the host function, and whether the two paths' flags agree. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GRID = 16
X0, Y0, SPAN = 412000.0, 5318000.0, 1010.0


def outline(vertices, seed=0):
    """→ polygons (lists of closed rings) with about ``vertices`` vertices in all."""
    rng = np.random.default_rng(seed)
    cell = SPAN / GRID
    taken = [(i, j) for i in range(GRID) for j in range(GRID) if (i // 2 + j // 2) % 2 == 0]
    seg = max(1, int(round(vertices / (4.0 * len(taken)))))
    corner = np.stack(np.meshgrid(np.arange(GRID + 1), np.arange(GRID + 1), indexing="ij"), axis=-1) * cell + rng.uniform(-0.2, 0.2, (GRID + 1, GRID + 1, 2)) * cell
    corner += np.array([X0, Y0])

    def border(a, b):                                    # a jagged line from corner a to corner b, its end left out
        t = np.arange(seg)[:, None] / seg
        line = a + t * (b - a)
        d = (b - a) / np.linalg.norm(b - a)
        line[1:] += np.stack([-d[1], d[0]]) * rng.uniform(-0.3, 0.3, (seg - 1, 1)) * min(1.0, cell / seg)
        return line

    hor = {(i, j): border(corner[i, j], corner[i + 1, j]) for i in range(GRID) for j in range(GRID + 1)}
    ver = {(i, j): border(corner[i, j], corner[i, j + 1]) for i in range(GRID + 1) for j in range(GRID)}
    back = lambda line, end: np.concatenate([end[None], line[:0:-1]])
    polygons = []
    for i, j in taken:
        ring = np.concatenate([hor[i, j], ver[i + 1, j], back(hor[i, j + 1], corner[i + 1, j + 1]), back(ver[i, j], corner[i, j + 1])])
        polygons.append([np.concatenate([ring, ring[:1]])])
    square = lambda c, h: np.array([[c[0] - h, c[1] - h], [c[0] + h, c[1] - h], [c[0] + h, c[1] + h], [c[0] - h, c[1] + h], [c[0] - h, c[1] - h]])
    for k in range(0, len(taken), 9):                    # clearings well inside a parcel, islands well inside a free cell
        i, j = taken[k]
        polygons[k].append(square(corner[i:i + 2, j:j + 2].reshape(-1, 2).mean(axis=0), 0.12 * cell))
    for i in range(GRID):
        for j in range(GRID):
            if (i // 2 + j // 2) % 2 == 1 and (i * GRID + j) % 11 == 0:
                polygons.append([square(corner[i:i + 2, j:j + 2].reshape(-1, 2).mean(axis=0), 0.1 * cell)])
    return polygons


def worker(path, n, vertices, reps):
    import clean_crowns_bench
    from treedetection_amd.vector import Region

    crowns, _ = clean_crowns_bench.scene(n)
    polygons = outline(vertices)
    res = {"outline_vertices": int(sum(len(r) for p in polygons for r in p)), "rings": int(sum(len(p) for p in polygons))}
    if path == "host":
        t = time.perf_counter()
        i, w = Region(polygons).relate(crowns)
        res["host_s"] = time.perf_counter() - t
    else:
        import torch
        from treedetection_amd import _lib

        torch.zeros(1, device="cuda").cpu()              # the context exists before the clock starts
        _lib.load()
        region = Region(polygons)
        t = time.perf_counter()
        i, w = region.relate(crowns, device=0)
        res["device_first_s"] = time.perf_counter() - t
        res["deferred"] = region.last_deferred
        t = time.perf_counter()
        i2, w2 = region.relate(crowns, device=0)
        res["device_again_s"] = time.perf_counter() - t
        assert i2.tolist() == i.tolist() and w2.tolist() == w.tolist()
        # the launch alone
        R = region._on_device[0]
        q_start = np.zeros(len(crowns) + 1, np.int64)
        q_start[1:] = np.cumsum([len(c) for c in crowns])
        d_q, d_qs = torch.from_numpy(np.concatenate(crowns)).cuda(), torch.from_numpy(q_start).cuda()
        d_f, d_s = torch.empty(len(crowns), dtype=torch.uint8, device="cuda"), torch.empty(len(crowns), dtype=torch.int32, device="cuda")
        ymin, ymax, inv_h = region._index[3:]
        lib, ms = _lib.load(), []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.td_region_relate_dev(R["xy"].data_ptr(), R["ring_start"].data_ptr(), R["ring_poly"].data_ptr(), region.n_rings,
                                                len(region.xy), R["edge_ring"].data_ptr(), R["bin_start"].data_ptr(), R["bin_edges"].data_ptr(),
                                                len(R["bin_start"]) - 1, R["n_bin_edges"], ymin, ymax, inv_h, d_q.data_ptr(), d_qs.data_ptr(),
                                                len(crowns), int(q_start[-1]), d_f.data_ptr(), d_s.data_ptr(), 0, _lib.stream_ptr()),
                       "td_region_relate_dev")
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res["launch_ms"] = statistics.median(ms[1:])
        res["device"] = torch.cuda.get_device_name(0)
    res["intersects"], res["within"] = int(i.sum()), int(w.sum())
    res["flags"] = (i.astype(np.uint8) | (w.astype(np.uint8) << 1)).tobytes().hex()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=["host", "device"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.n, args.sizes[0], args.reps)
    lines = [f"region_relate_bench: {args.n} crowns against an outline of adjacent parcels; seconds of wall clock, each path in its own process"]
    for size in args.sizes:
        got = {}
        for path in ("host", "device"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", path, "--n", str(args.n), "--sizes", str(size),
                                  "--reps", str(args.reps)], check=True, capture_output=True, text=True).stdout
            got[path] = json.loads(out.strip().splitlines()[-1])
        h, d = got["host"], got["device"]
        agree = h.pop("flags") == d.pop("flags")
        lines.append(f"outline {h['outline_vertices']:>8d} vertices, {h['rings']:>4d} rings: host {h['host_s']:.3f} s | device, fresh Region "
                     f"{d['device_first_s']:.3f} s, same Region again {d['device_again_s']:.3f} s, launch alone {d['launch_ms']:.3f} ms "
                     f"(median of {args.reps}) | deferred {d['deferred']} | intersects {h['intersects']}, within {h['within']} | "
                     f"flags {'agree' if agree else 'DIFFER'} | {d['device']}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
