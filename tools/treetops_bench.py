"""td_treetops_dev on a synthetic 5000 x 5000 canopy raster (seeded: crowns of 10 x 10 pixels with random heights, 30 % of them
ground, 2 m of noise) with the defaults (sigma 0.5: radius 2, window 7, floor 3.0). Per output set — marks only; marks and the smoothed
raster — the launch between HIP events on the stream: a warm-up, then the median, least and most of 30 launches; the bytes the launch
must move, rows * cols * (4 + 1 [+ 4]), over the median; and, from the tile shapes, the dwords a workgroup reads and writes in LDS over
the median. In children of their own: the host twin td_treetops on one thread, and scipy's three calls (gaussian_filter,
maximum_filter, argwhere) where scipy is installed — with the comparison of all three results.

    python tools/treetops_bench.py [--out profiles/treetops.txt]      # every step, each in a child process under its own `timeout`
    python tools/treetops_bench.py --step gpu                          # one step in this process: gpu | host | scipy

Prints one line per measurement and writes them to ``--out``."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

STEP_LIMIT = {"gpu": 180, "host": 300, "scipy": 300}             # seconds per step
SIDE, SIGMA, WINDOW, FLOOR = 5000, 0.5, 7, 3.0
WARMUP, REPEATS = 3, 30


def canopy():
    rng = np.random.default_rng(7)
    crowns = (rng.random((SIDE // 10, SIDE // 10)) * 30).astype(np.float32)
    crowns[rng.random(crowns.shape) < 0.3] = 0.0
    return np.ascontiguousarray(np.kron(crowns, np.ones((10, 10), np.float32)) + (rng.random((SIDE, SIDE)) * 2).astype(np.float32))


def lds_dwords_per_tile(r, h, tile=64):
    """Dword reads and writes of one workgroup in LDS, from the stages of treetops.hip."""
    e, e0 = tile + 2 * (r + h), tile + 2 * h
    reads = e0 * e * (2 * r + 1) + e0 * e0 * (2 * r + 1) + tile * e0 * (2 * h + 1) + tile * tile * (2 * h + 2)
    writes = e * e + e0 * e + e0 * e0 + tile * e0
    return reads + writes


def gpu_step():
    import torch
    from treedetection_amd import _lib, treetops as tt

    raster = canopy()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    w = tt.gaussian_weights(SIGMA)
    r, h = (w.size - 1) // 2, WINDOW // 2
    d_r = torch.from_numpy(raster).to(dev)
    d_m = torch.empty((SIDE, SIDE), dtype=torch.uint8, device=dev)
    d_s = torch.empty((SIDE, SIDE), dtype=torch.float32, device=dev)
    tiles = ((SIDE + 63) // 64) ** 2
    for what, smoothed in (("marks           ", None), ("marks + smoothed", d_s)):
        def launch():
            _lib.check(lib.td_treetops_dev(d_r.data_ptr(), SIDE, SIDE, w.ctypes.data, r, WINDOW, FLOOR, d_m.data_ptr(),
                                           smoothed.data_ptr() if smoothed is not None else None, None, _lib.stream_ptr()), "td_treetops_dev")
        for _ in range(WARMUP):
            launch()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(REPEATS)]
        for a, b in ev:
            a.record()
            launch()
            b.record()
        torch.cuda.synchronize()
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        med = float(np.median(us))
        moved = SIDE * SIDE * (4 + 1 + (4 if smoothed is not None else 0))
        lds = tiles * lds_dwords_per_tile(r, h) * 4
        print(f"gpu    {what}: median {med:.0f} us (least {us.min():.0f}, most {us.max():.0f}) of {REPEATS} launches after {WARMUP}; "
              f"{moved / 1e6:.0f} MB to move = {moved / med / 1e6:.2f} TB/s; {lds / 1e9:.2f} GB through LDS = {lds / med / 1e6:.1f} TB/s", flush=True)
    tops = int(d_m.sum().item())
    np.save(os.path.join(scratch(), "gpu_marks.npy"), np.packbits(d_m.cpu().numpy()))
    print(f"gpu    {tops} treetops on {SIDE} x {SIDE}, sigma {SIGMA}, window {WINDOW}, floor {FLOOR}", flush=True)


def scratch():
    d = os.environ.get("TREETOPS_BENCH_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin")
    os.makedirs(d, exist_ok=True)
    return d


def against_gpu(marks, who):
    path = os.path.join(scratch(), "gpu_marks.npy")
    if os.path.exists(path):
        same = np.array_equal(np.load(path), np.packbits(marks))
        print(f"{who} marks {'equal' if same else 'DIFFER FROM'} the GPU's", flush=True)


def host_step():
    from treedetection_amd import treetops as tt

    raster = canopy()
    t0 = time.perf_counter()
    marks = tt.treetop_marks(raster, SIGMA, WINDOW, FLOOR, device=None)
    dt = time.perf_counter() - t0
    print(f"host   td_treetops on one thread: {dt * 1e3:.0f} ms ({int(marks.sum())} treetops)", flush=True)
    against_gpu(marks, "host  ")


def scipy_step():
    try:
        import scipy
        import scipy.ndimage as nd
    except ImportError:
        print("scipy  not installed: not measured", flush=True)
        return
    raster = canopy()
    t0 = time.perf_counter()
    s = nd.gaussian_filter(raster, sigma=SIGMA)
    t1 = time.perf_counter()
    m = nd.maximum_filter(s, size=WINDOW)
    t2 = time.perf_counter()
    at = np.argwhere((s == m) & (s > np.float32(FLOOR)))
    t3 = time.perf_counter()
    print(f"scipy  {scipy.__version__}: gaussian_filter {(t1 - t0) * 1e3:.0f} ms + maximum_filter {(t2 - t1) * 1e3:.0f} ms + argwhere {(t3 - t2) * 1e3:.0f} ms "
          f"= {(t3 - t0) * 1e3:.0f} ms ({len(at)} treetops)", flush=True)
    marks = np.zeros(raster.shape, np.uint8)
    marks[at[:, 0], at[:, 1]] = 1
    against_gpu(marks, "scipy ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "treetops.txt"))
    args = ap.parse_args()
    if args.step:
        return {"gpu": gpu_step, "host": host_step, "scipy": scipy_step}[args.step]()
    lines = [f"# python tools/treetops_bench.py   (a seeded {SIDE} x {SIDE} canopy raster; sigma {SIGMA}, window {WINDOW}, floor {FLOOR})"]
    for step in ("gpu", "host", "scipy"):                        # a fresh child per step; a step that fails or runs out of time ends the run
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), "--step", step], check=False,
                           stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: stopping")
            return r.returncode
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
