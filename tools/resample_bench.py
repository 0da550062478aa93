"""The crown stage's two rasters, host path against device path, at a user's sizes:

  rgbi   10 000 x 10 000 four-band uint8, DEFLATE tiles, ndvi_scaling_factor 0.2 → float32 NDVI [2000, 2000] on the device
         host:   GeoTiff.read + resample_bilinear_gdal + ndvi_from_rgbi + copy to the device (the path of `device_decode: false`)
         device: GeoTiff.decode_to_device + td_resample_gdal_dev, mode ndvi                  (`device_decode: true`)
  ndsm   5 000 x 5 000 float32, DEFLATE tiles with the floating-point predictor, height_scaling_factor 0.5 → float32 [2500, 2500]
         host:   read + resample_bilinear_gdal + copy;   device: decode_to_device + td_resample_gdal_dev, mode f32

    python tools/resample_bench.py [--dir WORKDIR] [--out results.json] [--small]

The driver writes the two files (seeded, on the host), then runs every measurement as a child process of its own under `timeout`
and stops at the first one that fails. Each child prints one JSON line: wall times from the file to a synchronised device tensor
(every repeat listed; the first one of a process includes loading the kernels), and for the device path the time between HIP events
around the resampling call (tap tables built and uploaded + both kernels) and how many output values differ from the host path's
(saved by the host step)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5320000.0)
RASTERS = {"rgbi": dict(side=10000, factor=0.2), "ndsm": dict(side=5000, factor=0.5)}
STEPS = [("rgbi", "host", 900), ("rgbi", "device", 300), ("ndsm", "host", 600), ("ndsm", "device", 300)]      # (raster, path, time limit in s)


def make_files(workdir, small):
    from treedetection_amd.geotiff import write_geotiff
    rng = np.random.default_rng(0)
    for name, r in RASTERS.items():
        side = r["side"] // 10 if small else r["side"]
        path = os.path.join(workdir, f"{name}.tif")
        cells = side // 100
        if name == "rgbi":                                 # 100-pixel patches with three bits of noise: compresses like an orthophoto, not like noise
            img = np.repeat(np.repeat(rng.integers(0, 248, (4, cells, cells), dtype=np.uint8), 100, axis=1), 100, axis=2)
            img += rng.integers(0, 8, img.shape, dtype=np.uint8)
            write_geotiff(path, img, T, 25832, compression="deflate", tile=(512, 512))
        else:
            img = np.repeat(np.repeat(rng.uniform(0, 30, (cells, cells)).astype(np.float32), 100, axis=0), 100, axis=1)
            img += rng.uniform(0, 0.5, img.shape).astype(np.float32)
            write_geotiff(path, img[None], T, 25832, compression="deflate", predictor=3, tile=(512, 512))
        print(f"{path}: {side} x {side}, {os.path.getsize(path) / 1e6:.0f} MB", flush=True)


def step(workdir, name, path_kind, repeats):
    import torch
    from treedetection_amd import postprocessing as P
    from treedetection_amd.geotiff import GeoTiff
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    tif, saved = os.path.join(workdir, f"{name}.tif"), os.path.join(workdir, f"{name}_host.npy")
    factor = RASTERS[name]["factor"]
    walls, kernel_ms, parts = [], [], {}
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = GeoTiff(tif)
        out_h, out_w = int(g.height * factor), int(g.width * factor)
        if path_kind == "host":
            raw = g.read() if name == "rgbi" else g.read()[:1]
            t1 = time.perf_counter()
            res = P.resample_bilinear_gdal(raw, out_h, out_w)
            t2 = time.perf_counter()
            arr = P.ndvi_from_rgbi(res).astype(np.float32) if name == "rgbi" else res[0].astype(np.float32)
            t3 = time.perf_counter()
            out = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            parts = {"read_s": t1 - t0, "resample_s": t2 - t1, "ndvi_s": t3 - t2, "h2d_s": t4 - t3}
        else:
            _, check = g.decode_to_device(dev)
            image = check()
            t1 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "rgbi":
                out = P.resample_on_device(image, out_h, out_w, [0, 3], "ndvi")
            else:
                out = P.resample_on_device(image.view(g.height, g.width), out_h, out_w, [0], "f32")[0]
            b.record()
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            kernel_ms.append(a.elapsed_time(b))            # (HIP events around building + uploading the tap tables and the two kernels)
            parts = {"decode_s": t1 - t0, "tables_and_resample_s": t4 - t1, "decode_kernel_ms": check.kernel_ms}
        walls.append(t4 - t0)
        g.close()
    line = {"raster": name, "path": path_kind, "shape": [g.height, g.width], "out": [out_h, out_w], "wall_s": [round(w, 4) for w in walls],
            "last_repeat": {k: round(v, 4) for k, v in parts.items()}}
    if path_kind == "host":
        np.save(saved, out.cpu().numpy())
    else:
        line["tables_and_resample_ms"] = [round(v, 3) for v in kernel_ms]
        if os.path.exists(saved):
            want, got = np.load(saved), out.cpu().numpy()
            line["values_differing_from_host"] = int((want.view(np.uint32) != got.view(np.uint32)).sum())
            line["largest_difference"] = float(np.abs(want.astype(np.float64) - got).max())
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the two rasters are written (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="write the result lines to this JSON file too")
    ap.add_argument("--small", action="store_true", help="a tenth of the side lengths (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--step", nargs=2, metavar=("RASTER", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.dir, args.step[0], args.step[1], repeats=2 if args.step[1] == "host" else 4)
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        workdir = args.dir or tmp
        os.makedirs(workdir, exist_ok=True)
        make_files(workdir, args.small)
        results = []
        for name, path_kind, limit in STEPS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--dir", workdir, "--step", name, path_kind]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                print(f"{name} / {path_kind} ended with status {r.returncode}: stopping here", flush=True)
                return r.returncode
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
