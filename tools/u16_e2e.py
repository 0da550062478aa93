"""Files-to-files Predictor rate on a 16-bit orthophoto, host reader (false: every window read, rescaled in float64 and copied to the
device per tile) against the device path (true: the raster decoded into HBM as uint16, windows turned into the model input there):
python tools/u16_e2e.py [side=9000] [tile=256] [codec=lzw|deflate|none] [predictor=2] [precision=fp32] [batch=8] [images=3]
[modes=false,true] [rounds=2]
The raster (side x side x 3 uint16 = synthetic orthophoto tiles x 257, so the reference's 255 * x / 65535 rule applies) is cut into the
reference's 450 x 450 px tiles; every mode predicts one warm-up image, then `images` images back to back as
detection.predict_on_model walks them (the next one prefetched while the current one predicts); the modes alternate in one process.
codec=none stores the samples uncompressed (then `true` means "all": the raster is uploaded whole). Prints one JSON line: tiles/s per
mode, the decode stats, and whether the Prediction_*.json files are identical."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import treedetection_amd as T                                      # noqa: E402
from treedetection_amd.geotiff import write_geotiff               # noqa: E402
from treedetection_amd.preprocessing import tile_data             # noqa: E402
from treedetection_amd.synth import make_tile                      # noqa: E402
from treedetection_amd.weights import make_synthetic_state_dict   # noqa: E402

args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
side, tile, nimg = int(args.get("side", 9000)), int(args.get("tile", 256)), int(args.get("images", 3))
codec = args.get("codec", "lzw")
modes = [m if m in ("auto", "all") else (m == "true" and ("all" if codec == "none" else True)) for m in args.get("modes", "false,true").split(",")]
base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
root = tempfile.mkdtemp(prefix="td_u16_e2e_", dir=base)
try:
    os.makedirs(f"{root}/rgb")
    S = 1000
    n = -(-side // S)
    tiles = [make_tile(i, S)[0] for i in range(min(16, n * n))]
    img = np.zeros((3, n * S, n * S), np.uint16)
    for r in range(n):
        for c in range(n):
            img[:, r * S:(r + 1) * S, c * S:(c + 1) * S] = tiles[(r * n + c) % len(tiles)].transpose(2, 0, 1).astype(np.uint16) * 257
    img = np.ascontiguousarray(img[:, :side, :side])
    tif = f"{root}/rgb/324125000.tif"
    layout = {} if codec == "none" else {"compression": codec, "tile": (tile, tile), "predictor": int(args.get("predictor", 2))}
    write_geotiff(tif, img, (0.2, 0.0, 412000.0, 0.0, -0.2, 5318000.0 + side * 0.2), 25832, **layout)
    del img
    tile_data([tif], f"{root}/tiles", buffer=0, tile_width=90, tile_height=90)
    tjson = f"{root}/tiles/324125000.json"
    ntiles = len(json.load(open(tjson)))
    names = [str(324125001 + k) for k in range(nimg)]
    for nm in names:
        os.link(tif, f"{root}/rgb/{nm}.tif")
        os.link(tjson, f"{root}/tiles/{nm}.json")
    sd = make_synthetic_state_dict(int(args.get("depth", 50)), seed=0)
    cfg = T.setup_model_cfg(update_model="synthetic", device="0")
    precision, batch = args.get("precision", "fp32"), int(args.get("batch", 8))
    res = {"raster": f"{side}x{side}x3 uint16 {codec}" + ("" if codec == "none" else f", {tile}x{tile} tiles, predictor {layout['predictor']}"),
           "tiles_per_image": ntiles, "file_bytes": os.path.getsize(tif), "precision": precision, "batch": batch}
    outs = {}
    for rnd in range(int(args.get("rounds", 2))):          # the modes alternate: false, true, false, true — the rounds show the spread
        for dd in modes:
            out = f"{root}/out_{dd}"
            pred = T.Predictor(cfg, device_type="0", max_batch_size=batch, output_dir=out, precision=precision,
                               state_dict=sd, return_predictions=False, device_decode=dd)
            try:
                pred.prefetch(tif)
                pred(tif, tjson)                               # warm-up image
                warm = dict(pred.upload_stats if dd == "all" else pred.decode_stats)
                t0 = time.perf_counter()
                pending = None
                pred.prefetch(f"{root}/rgb/{names[0]}.tif")
                for k, nm in enumerate(names):
                    if k + 1 < len(names):
                        pred.prefetch(f"{root}/rgb/{names[k + 1]}.tif")
                    h = pred.submit(f"{root}/rgb/{nm}.tif", f"{root}/tiles/{nm}.json")
                    if pending is not None:
                        pending.result()
                    pending = h
                pending.result()
                dt = time.perf_counter() - t0
                files = sorted(os.listdir(f"{out}/{names[0]}"))
                assert len(files) == ntiles, (dd, len(files))
                outs[f"{dd}/{rnd}"] = {f: open(f"{out}/{names[0]}/{f}", "rb").read() for f in files}
                r = res.setdefault(f"device_decode={dd}", {"unit": "tiles/s", "images": len(names), "rounds": [], "seconds": []})
                r["rounds"].append(len(names) * ntiles / dt)
                r["seconds"].append(dt)
                r["value"] = sum(r["rounds"]) / len(r["rounds"])
                st = dict(pred.upload_stats if dd == "all" else pred.decode_stats)        # of the timed images (the warm-up's taken off)
                r["decode"] = {k: v - warm.get(k, 0) for k, v in st.items()}
            finally:
                pred.close()
                shutil.rmtree(out, ignore_errors=True)
    vals = list(outs.values())
    res["prediction_files_identical"] = all(v == vals[0] for v in vals)
    print(json.dumps(res))
finally:
    shutil.rmtree(root, ignore_errors=True)
