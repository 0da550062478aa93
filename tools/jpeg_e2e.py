"""Files-to-files Predictor rate on a JPEG-in-TIFF raster, device decoder on ("auto" / true) against the host reader (false):
python tools/jpeg_e2e.py [codec=jpeg | zstd [level=9] | lzw | deflate, the three with [predictor=2]] [side=9000] [tile=256] [quality=90] [subsampling=2] [layout=complete|gdal] [restart=0] [precision=fp16]
[batch=16] [images=3] [modes=true,false] [bands=3|4] [device_decode_long_jpeg=false|true]
The raster (side x side x bands uint8, synthetic orthophoto tiles; bands=4 adds the green band again as a near-infrared band: RGBI,
of which the tile loop reads bands 0 - 2) is cut into the reference's 450 x 450 px tiles; every mode predicts
one warm-up image, then `images` images back to back as detection.predict_on_model walks them (the next one prefetched while the
current one predicts). ``device_decode_long_jpeg=true`` passes the config key of that name: a raster without restart markers, which the
device modes otherwise leave to the host reader, is decoded on the device with a wave per entropy-coded segment. Prints one JSON line: tiles/s per mode, the decode stats, and whether the Prediction_*.json files are identical."""
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
side, tile, nimg, bands = int(args.get("side", 9000)), int(args.get("tile", 256)), int(args.get("images", 3)), int(args.get("bands", 3))
modes = [m if m in ("auto", "all") else m == "true" for m in args.get("modes", "true,false").split(",")]
long_jpeg = args.get("device_decode_long_jpeg", "false")
base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
root = tempfile.mkdtemp(prefix="td_jpeg_e2e_", dir=base)
try:
    os.makedirs(f"{root}/rgb")
    S = 1000
    n = -(-side // S)
    tiles = [make_tile(i, S)[0] for i in range(min(16, n * n))]
    img = np.zeros((bands, n * S, n * S), np.uint8)
    for r in range(n):
        for c in range(n):
            t = tiles[(r * n + c) % len(tiles)].transpose(2, 0, 1)
            img[:, r * S:(r + 1) * S, c * S:(c + 1) * S] = t if bands == 3 else np.concatenate([t, t[1:2]])
    img = np.ascontiguousarray(img[:, :side, :side])
    tif = f"{root}/rgb/324125000.tif"
    codec = args.get("codec", "jpeg")
    if codec == "jpeg":
        ckw = dict(jpeg_quality=int(args.get("quality", 90)), jpeg_subsampling=int(args.get("subsampling", 2)),
                   jpeg_tables=args.get("layout", "complete") == "gdal", jpeg_restart=int(args.get("restart", 0)))
    else:                                                          # a lossless codec of the block decoders
        ckw = dict(predictor=int(args.get("predictor", 2)), **({"zstd_level": int(args.get("level", 9))} if codec == "zstd" else {}))
    write_geotiff(tif, img, (0.2, 0.0, 412000.0, 0.0, -0.2, 5318000.0 + side * 0.2), 25832, compression=codec, tile=(tile, tile), **ckw)
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
    res = {"raster": f"{side}x{side}x{bands} uint8 {codec.upper()}, {tile}x{tile} tiles", "tiles_per_image": ntiles, "file_bytes": os.path.getsize(tif),
           "precision": args.get("precision", "fp16"), "device_decode_long_jpeg": long_jpeg}
    outs = {}
    for dd in modes:
        out = f"{root}/out_{dd}"
        pred = T.Predictor(cfg, device_type="0", max_batch_size=int(args.get("batch", 16)), output_dir=out, precision=args.get("precision", "fp16"),
                           state_dict=sd, return_predictions=False, device_decode=dd, device_decode_long_jpeg=long_jpeg)
        try:
            pred.prefetch(tif)
            pred(tif, tjson)                               # warm-up image
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
            outs[str(dd)] = {f: open(f"{out}/{names[0]}/{f}", "rb").read() for f in files}
            res[f"device_decode={dd}"] = {"value": len(names) * ntiles / dt, "unit": "tiles/s", "images": len(names), "seconds": dt,
                                          "decode": dict(pred.decode_stats)}
        finally:
            pred.close()
            shutil.rmtree(out, ignore_errors=True)
    vals = list(outs.values())
    res["prediction_files_identical"] = all(v == vals[0] for v in vals)
    print(json.dumps(res))
finally:
    shutil.rmtree(root, ignore_errors=True)
