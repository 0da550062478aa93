"""What the seam strips of ``use_overlap`` cost with ``device_seams`` off and on (treedetection_amd/merging.py, csrc/seam.hip):
python tools/seam_bench.py [side=9000] [limit=600]                                   — every configuration below, one JSON line each
python tools/seam_bench.py samples=u8|f32 codec=lzw|deflate tile=256|strip=8 [side=9000]   — one configuration, one JSON line
A 2 x 2 grid of side x side rasters — samples=u8: four uint8 bands (RGBI, predictor 2); samples=f32: one float32 band (a synthetic
nDSM, predictor 3) — as LZW and DEFLATE, in 256 x 256 tiles and in 8-row strips; tile_width 1000, buffer 100, overlapping_tiles 3: four
seams, two strips of 3 600 x side px and two of side x 3 600 px. The four rasters hold the same pixels (one is encoded, the others are
copies with their origin patched): the stage never compares neighbours, and encoding is not what is measured.
Per configuration: the wall time of ``merge_and_crop_images`` with the key off (today's path: both rasters decoded whole on the host,
the union mosaic, the centre crop) and on, in turns, on the same files in /dev/shm, page cache warm; the strip files of both are compared
byte for byte; and td_seam_first_dev alone on the covers of one seam of either orientation — HIP events around the launch, median of
7 warm runs, with the bytes it moves (one read of each source rectangle, one write of the strip) over that time.
Without ``samples=`` the configurations run one after the other, each in a process of its own under a time limit of ``limit`` seconds,
and the run ends at the first that fails or runs out of time: nothing is started on a GPU after a fault."""
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
CONFIGS = [(s, c, l) for s in ("u8", "f32") for c in ("lzw", "deflate") for l in ("tile=256", "strip=8")]


def every_configuration():
    side, limit = args.get("side", "9000"), int(args.get("limit", 600))
    for samples, codec, layout in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), f"samples={samples}", f"codec={codec}", layout, f"side={side}"]
        try:
            r = subprocess.run(cmd, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{' '.join(cmd[2:])}: no result within {limit} s — stopping here")
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd[2:])}: exit code {r.returncode} — stopping here")


if "samples" not in args:
    every_configuration()
    sys.exit(0)

import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from treedetection_amd import _lib                                # noqa: E402
from treedetection_amd import merging as M                        # noqa: E402
from treedetection_amd.geotiff import GeoTiff, write_geotiff      # noqa: E402
from treedetection_amd.synth import make_tile                     # noqa: E402


class Log:
    def __init__(self):
        self.errors = []

    def error(self, m):
        self.errors.append(m)

    def __getattr__(self, name):
        return lambda m: None


def grid(d, samples, codec, kw, side, gsd=0.2):
    """The four rasters of the grid in folder ``d`` → their paths. One raster is encoded; its three neighbours are the same bytes with
    the six doubles of the ModelTiepoint tag replaced."""
    n = -(-side // 1000)
    tiles = [make_tile(i, 1000) for i in range(min(16, n * n))]
    if samples == "u8":
        img = np.zeros((4, n * 1000, n * 1000), np.uint8)
        for r in range(n):
            for c in range(n):
                t = tiles[(r * n + c) % len(tiles)][0]
                img[:3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t.transpose(2, 0, 1)
                img[3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t[..., 1]
        img, predictor = np.ascontiguousarray(img[:, :side, :side]), 2
    else:
        img = np.ascontiguousarray(np.block([[tiles[(r * n + c) % len(tiles)][1] for c in range(n)] for r in range(n)])[None, :side, :side])
        img, predictor = img.astype(np.float32), 3
    x0, y0 = 412000.0, 5318000.0
    first = os.path.join(d, "1000_x.tif")
    write_geotiff(first, img, (gsd, 0, x0, 0, -gsd, y0), 25832, compression=codec, predictor=predictor, **kw)
    raw = open(first, "rb").read()
    tie = struct.pack("<6d", 0.0, 0.0, 0.0, x0, y0, 0.0)
    assert raw.count(tie) == 1
    paths = [first]
    for k, (ix, iy) in enumerate(((1, 0), (0, 1), (1, 1)), 1):
        paths.append(os.path.join(d, f"{1000 + k}_x.tif"))
        with open(paths[-1], "wb") as f:
            f.write(raw.replace(tie, struct.pack("<6d", 0.0, 0.0, 0.0, x0 + ix * side * gsd, y0 - iy * side * gsd, 0.0)))
    return paths, img.nbytes, len(raw)


def launch_alone(first, second, horizontal, config):
    """td_seam_first_dev on the covers of one pair, as merging._cut_on_device launches it → (ms of 7 warm launches, bytes moved)."""
    a, b = GeoTiff(first), GeoTiff(second)
    geo = M.seam_windows(a, b, horizontal, config)
    _, _, rows, cols = geo.strip
    px = a.count * a.dtype.itemsize
    keep, sources, moved = [], [], rows * cols * px
    for src, part in zip((a, b), geo.sources):
        (window, (at_row, at_col)) = part
        cover, check = src.decode_to_device("cuda:0", window=window)
        check()
        wr, wc, h, w = check.window
        keep.append(cover)
        moved += h * w * px
        sources.append(_lib.SeamSource(data=cover.data_ptr(), pitch=cover.shape[1], rows=cover.shape[0], row0=at_row - wr, col0=at_col - wc,
                                       r_lo=at_row, c_lo=at_col, r_hi=at_row + h, c_hi=at_col + w, has_own=0, own=0.0))
    strip = torch.empty((rows * cols * px,), dtype=torch.uint8, device="cuda")
    lib, sample = _lib.load(), M._SEAM_DTYPES[np.dtype(a.dtype.newbyteorder("="))]
    ms = []
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.td_seam_first_dev(strip.data_ptr(), rows, cols, a.count, sample, float(geo.fill), sources[0], sources[1], _lib.stream_ptr()),
                   "td_seam_first_dev")
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[1:], moved, (rows, cols)


def main():
    samples, codec, side = args["samples"], args["codec"], int(args.get("side", 9000))
    kw = {"rows_per_strip": int(args["strip"])} if "strip" in args else {"tile": (int(args.get("tile", 256)),) * 2}
    base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="td_seambench_", dir=base)
    try:
        t0 = time.perf_counter()
        paths, raw_bytes, file_bytes = grid(d, samples, codec, kw, side)
        t_write = time.perf_counter() - t0
        torch.cuda.init()
        torch.zeros(1, device="cuda")
        wall, files = {False: [], True: []}, {}
        for turn in range(2):
            for on in (False, True):
                config = {"logger": Log(), "merged_path": f"merged_{on}", "tile_width": 1000, "tile_height": 1000, "buffer": 100,
                          "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "device_seams": on}
                lists = (list(paths), []) if samples == "u8" else ([], list(paths))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.merge_and_crop_images(config, *lists)
                torch.cuda.synchronize()
                wall[on].append(time.perf_counter() - t0)
                new = (lists[0] if samples == "u8" else lists[1])[4:]
                assert len(new) == 4 and not config["logger"].errors, config["logger"].errors
                if turn == 0:
                    files[on] = [open(p, "rb").read() for p in new]
                shutil.rmtree(os.path.join(d, f"merged_{on}"))
        assert files[False] == files[True], "the device strips differ from the host strips"
        strip_bytes = sum(len(b) for b in files[True])
        del files
        line = {"samples": samples, "codec": codec, "layout": kw, "raster": f"{side}x{side}x{4 if samples == 'u8' else 1}", "rasters": 4, "strips": 4,
                "raw_mb_per_raster": raw_bytes / 1e6, "file_mb_per_raster": file_bytes / 1e6, "strip_mb_written": strip_bytes / 1e6,
                "encode_one_raster_s": round(t_write, 1), "device_seams_off_s": [round(t, 3) for t in wall[False]],
                "device_seams_on_s": [round(t, 3) for t in wall[True]], "strips_identical": True,
                "off_over_on": round(min(wall[False]) / min(wall[True]), 2)}
        config = {"tile_width": 1000, "tile_height": 1000, "buffer": 100, "overlapping_tiles_width": 3, "overlapping_tiles_height": 3}
        for name, horizontal, other in (("tall", True, paths[1]), ("flat", False, paths[2])):
            ms, moved, shape = launch_alone(paths[0], other, horizontal, config)
            line[f"kernel_{name}_strip"] = {"rows_cols": shape, "ms": [round(t, 4) for t in ms], "median_ms": round(median(ms), 4),
                                            "gb_per_s_read_plus_write": round(moved / (median(ms) * 1e-3) / 1e9, 1)}
        print(json.dumps(line), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


main()
