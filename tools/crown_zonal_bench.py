"""td_crown_zonal_dev beside td_crown_stats on the inputs of tools/crown_bench.py: a 5000 x 5000 NDVI raster (0.2 m), a 1000 x 1000
nDSM (1 m) and 20 000 crowns of 1.5 - 6 m radius — the circles of crown_bench.py for the circle kernel, star-shaped rings of 20 - 60
vertices around the same centres (vertex radii 0.6 - 1.0 of the circle's) for the zonal kernel. Times, per raster: the zonal launch,
the circle launch of the unchanged td_crown_stats on the same crowns (HIP events, 10 launches after a warm-up) and the host twin
td_crown_zonal on one thread.

    python tools/crown_zonal_bench.py                  # every step in a child process of its own, each under its own `timeout`
    python tools/crown_zonal_bench.py --step zonal     # one step in this process: zonal | circle | host

Prints one line per step and raster; writes nothing."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

N = 20000
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5319000.0)
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5319000.0)
STEP_LIMIT = {"zonal": 120, "circle": 120, "host": 300}          # seconds per step


def inputs():
    rng = np.random.default_rng(0)                               # (the draws of crown_bench.py, in its order)
    ndvi = rng.uniform(-0.2, 0.9, (5000, 5000)).astype(np.float32)
    ndsm = rng.uniform(0, 30, (1000, 1000)).astype(np.float32)
    cx, cy, r = rng.uniform(412010, 412990, N), rng.uniform(5318010, 5318990, N), rng.uniform(1.5, 6.0, N)
    circles = np.stack([cx, cy, r], axis=1).astype(np.float32)
    rings = []
    for k in range(N):
        m = int(rng.integers(20, 61))
        ang = (np.arange(m) + rng.uniform(0.1, 0.9, m)) * (2 * np.pi / m)
        rad = r[k] * rng.uniform(0.6, 1.0, m)
        rings.append(np.stack([cx[k] + rad * np.cos(ang), cy[k] + rad * np.sin(ang)], axis=1))
    return (("ndvi 5000x5000", ndvi, T, 1), ("ndsm 1000x1000", ndsm, NT, 0)), circles, rings


def gpu_step(step):
    import torch
    from treedetection_amd import _lib
    from treedetection_amd.cleaning import pack_rings

    rasters, circles, rings = inputs()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    xy, start = pack_rings(rings)
    d_xy, d_st, d_c = torch.from_numpy(xy).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(circles).to(dev)
    for name, raster, tr, mode in rasters:
        d_r = torch.from_numpy(raster).to(dev)
        trc = (C.c_double * 6)(*tr)
        if step == "zonal":
            d_o, d_p, d_s = (torch.empty((N, 4), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.int32, device=dev),
                             torch.empty(N, dtype=torch.int32, device=dev))
            call = lambda: _lib.check(lib.td_crown_zonal_dev(d_r.data_ptr(), raster.shape[0], raster.shape[1], trc, d_xy.data_ptr(), xy.shape[0],
                                                             d_st.data_ptr(), N, d_o.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), _lib.stream_ptr()), "zonal")
        else:
            d_o = torch.empty((N, 4 if mode else 3), dtype=torch.float32, device=dev)
            win = (C.c_int32 * 4)(0, 0, raster.shape[0] - 1, raster.shape[1] - 1)
            call = lambda: _lib.check(lib.td_crown_stats(d_r.data_ptr(), raster.shape[0], raster.shape[1], trc, win, d_c.data_ptr(), N, mode, 1.0,
                                                         d_o.data_ptr(), _lib.stream_ptr()), "circle")
        call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            call()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / 10 * 1e3
        extra = ""
        if step == "zonal":
            cnt = d_p[:, 0].cpu().numpy()
            assert (d_s.cpu().numpy() == 0).all()
            extra = f", {int(cnt.sum())} pixels inside ({cnt.mean():.1f} per crown), {xy.shape[0]} vertices"
        print(f"{step:6s} {name}: {us:.0f} us for {N} crowns{extra}", flush=True)


def host_step():
    from treedetection_amd import postprocessing as P
    from treedetection_amd.cleaning import pack_rings

    rasters, _, rings = inputs()
    packed = pack_rings(rings)
    for name, raster, tr, _ in rasters:
        t0 = time.perf_counter()
        _, count, _, status = P.crown_zonal_stats(raster, tr, None, device=None, packed=packed)
        dt = time.perf_counter() - t0
        assert (status == 0).all()
        print(f"host   {name}: {dt * 1e3:.0f} ms for {N} crowns on one thread ({int(count.sum())} pixels inside)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT))
    args = ap.parse_args()
    if args.step:
        return host_step() if args.step == "host" else gpu_step(args.step)
    for step in ("zonal", "circle", "host"):                     # a fresh child per step; a step that fails or runs out of time ends the run
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), "--step", step], check=False)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: stopping")
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
