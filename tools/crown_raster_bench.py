"""td_crown_labels_dev beside td_crown_zonal_dev on the inputs of tools/crown_zonal_bench.py: 20 000 star-shaped rings of 20 - 60
vertices on the 5000 x 5000 raster of 0.2 m pixels and on the 1000 x 1000 raster of 1 m pixels. Values: the distinct priorities
crown_priorities gives seeded scores. Times, per raster, in ONE process with the launches alternating: the label launch on a raster
cleared before every launch (HIP events around the launch alone), the clear on its own, the zonal launch on the same rings — mean,
least and most of 10 launches after a warm-up — and, in a child of its own, the host twin td_crown_labels on one thread. Also what
the launch draws: pixels that get a label, the per-crown pixel total, and the share of labelled pixels that more than one crown
covers (the winner under the priorities differs from the winner under the reversed priorities exactly there).

    python tools/crown_raster_bench.py                 # both steps, each in a child process of its own under its own `timeout`
    python tools/crown_raster_bench.py --step gpu      # one step in this process: gpu | host

Prints one line per measurement and raster; writes nothing."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from crown_zonal_bench import N, inputs  # noqa: E402

STEP_LIMIT = {"gpu": 180, "host": 300}                           # seconds per step
REPEATS = 10


def priorities():
    from treedetection_amd import postprocessing as P
    return P.crown_priorities(np.random.default_rng(1).integers(30, 100, N) / 100.0)[0]       # scores with many ties


def gpu_step():
    import torch
    from treedetection_amd import _lib
    from treedetection_amd.cleaning import pack_rings

    rasters, _, rings = inputs()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    xy, start = pack_rings(rings)
    prio = priorities()
    d_xy, d_st = torch.from_numpy(xy).to(dev), torch.from_numpy(start).to(dev)
    d_v = torch.from_numpy(prio.view(np.int32)).to(dev)
    d_w = torch.from_numpy((np.uint32(N + 1) - prio).view(np.int32)).to(dev)                  # the reversed priorities
    for name, raster, tr, _ in rasters:
        rows, cols = raster.shape
        d_r = torch.from_numpy(raster).to(dev)
        trc = (C.c_double * 6)(*tr)
        d_l = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
        d_s = torch.empty(N, dtype=torch.int32, device=dev)
        d_o, d_p, d_zs = (torch.empty((N, 4), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.int32, device=dev),
                          torch.empty(N, dtype=torch.int32, device=dev))

        def labels(values=d_v, out=d_l):
            _lib.check(lib.td_crown_labels_dev(rows, cols, trc, d_xy.data_ptr(), xy.shape[0], d_st.data_ptr(), values.data_ptr(), N, out.data_ptr(),
                                               d_s.data_ptr(), _lib.stream_ptr()), "labels")

        def zonal():
            _lib.check(lib.td_crown_zonal_dev(d_r.data_ptr(), rows, cols, trc, d_xy.data_ptr(), xy.shape[0], d_st.data_ptr(), N, d_o.data_ptr(),
                                              d_p.data_ptr(), d_zs.data_ptr(), _lib.stream_ptr()), "zonal")

        for _ in range(2):                                       # warm-up: every launch the timed window uses
            d_l.zero_()
            labels()
            zonal()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(REPEATS)]
        for e in ev:                                             # clear | label launch | zonal launch, alternating
            e[0].record()
            d_l.zero_()
            e[1].record()
            labels()
            e[2].record()
            zonal()
            e[3].record()
        torch.cuda.synchronize()
        us = np.array([[e[k].elapsed_time(e[k + 1]) * 1e3 for k in range(3)] for e in ev])
        assert (d_s.cpu().numpy() == 0).all() and (d_zs.cpu().numpy() == 0).all()
        inside = int(d_p[:, 0].sum().item())
        d_m = torch.zeros_like(d_l)
        labels(d_w, d_m)
        torch.cuda.synchronize()
        labelled = int((d_l != 0).sum().item())
        shared = int(((d_l != 0) & (d_l + d_m != N + 1)).sum().item())         # the two winners differ: more than one crown
        for k, what in enumerate(("clear ", "labels", "zonal ")):
            print(f"{what} {name}: {us[:, k].mean():.0f} us (least {us[:, k].min():.0f}, most {us[:, k].max():.0f}) over {REPEATS} launches for {N} crowns",
                  flush=True)
        print(f"drawn  {name}: {inside} atomics (pixels inside, summed over the crowns), {labelled} pixels labelled = {100.0 * labelled / (rows * cols):.1f} % "
              f"of the raster, {shared} of them = {100.0 * shared / max(labelled, 1):.1f} % covered by more than one crown", flush=True)


def host_step():
    from treedetection_amd import postprocessing as P
    from treedetection_amd.cleaning import pack_rings

    rasters, _, rings = inputs()
    packed = pack_rings(rings)
    prio = priorities()
    for name, raster, tr, _ in rasters:
        t0 = time.perf_counter()
        labels, status = P.crown_label_raster(None, prio, tr, raster.shape, device=None, packed=packed)
        dt = time.perf_counter() - t0
        assert (status == 0).all()
        print(f"host   {name}: {dt * 1e3:.0f} ms for {N} crowns on one thread ({int((labels != 0).sum())} pixels labelled)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT))
    args = ap.parse_args()
    if args.step:
        return host_step() if args.step == "host" else gpu_step()
    for step in ("gpu", "host"):                                 # a fresh child per step; a step that fails or runs out of time ends the run
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), "--step", step], check=False)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: stopping")
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
