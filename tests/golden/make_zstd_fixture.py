"""Writes tests/golden/zstd: Zstandard frames as libzstd wrote them (both builds this machine has: the system's and Pillow's bundled
one), the hand-built frames of zstd_cases.hand_frames() (hand_*.zst), five small ZSTD GeoTIFFs, and manifest.json (per stream: name, file, libzstd version, level, decoded length, SHA-256; decoded
payloads only for streams under 4 KB). Asserts through td_zstd_stream_stats that the streams reach every mode of
zstd_cases.REQUIRED_MODES, no file is above 560 KB and the directory stays under 1.5 MB. Run from the repository root with the
library built:  python tests/golden/make_zstd_fixture.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import zstd_cases as zc  # noqa: E402

FILE_MAX, DIR_MAX = 560 << 10, 1536 << 10


def file_rasters():
    """name → (array [bands, rows, cols], write_geotiff options): the whole-file fixtures."""
    img = zc.smooth_image(seed=21, side=256, bands=4, noise=0.0)[:150, :200].astype(np.int64)
    chw = img.transpose(2, 0, 1)
    f32 = (chw[0] * 0.173 + np.linspace(0, 9, 200)[None, :]).astype(np.float32)
    return {
        "rgb_tiles_p2": (chw[:3].astype(np.uint8), dict(tile=(64, 64), predictor=2)),
        "rgbi_strips7": ((chw // 8 * 8).astype(np.uint8), dict(rows_per_strip=7)),      # (coarse levels: strips without a predictor stay under 100 KB)
        "rgb16_tiles_p2": ((chw[:3] * 197 + 1000).astype(np.uint16), dict(tile=(64, 64), predictor=2)),
        "f32_tiles_p3": (f32, dict(tile=(64, 64), predictor=3)),
    }


def main():
    from treedetection_amd.geotiff import GeoTiff, write_geotiff
    builds = {z.version: z for z in zc.libzstd_builds()}
    assert len(builds) >= 2, f"two libzstd builds are needed, found {sorted(builds)}"
    old, new = (builds[v] for v in sorted(builds, key=lambda s: tuple(int(x) for x in s.split(".")))[:2])
    ins = zc.inputs()
    os.makedirs(zc.GOLDEN, exist_ok=True)
    for f in os.listdir(zc.GOLDEN):
        os.remove(os.path.join(zc.GOLDEN, f))
    plan = []                                                       # (name, input, build, level, how)
    for i, name in enumerate(k for k in ins if not k.startswith("period")):
        plan.append((f"{name}_l9", name, (old, new)[i % 2], 9, "oneshot"))
    for z in (old, new):
        tag = "old" if z is old else "new"
        for lvl in (1, 19):
            plan.append((f"labels_l{lvl}_{tag}", "labels", z, lvl, "oneshot"))
        if z is new:
            plan.append((f"image16_l3_{tag}", "image16", z, 3, "oneshot"))
        plan.append((f"image64_diff_l1_{tag}", "image64_diff", z, 1, "oneshot"))
    plan.append(("image64_checksum", "image64", new, 3, "checksum"))
    plan.append(("labels_stream", "labels", new, 3, "stream"))
    plan.append(("image64_stream_old", "image64", old, 9, "stream4000"))       # (chunks smaller than the input: a window descriptor)
    for p in zc.PERIODS:
        plan.append((f"period{p}_700", f"period{p}_700", (old, new)[p % 2], 9, "oneshot"))
    plan.append(("period7_210000", "period7_210000", new, 9, "oneshot"))
    streams, reached = [], {}
    for name, key, z, lvl, how in plan:
        data = ins[key]
        s = {"oneshot": lambda: z.compress(data, lvl), "checksum": lambda: z.compress_advanced(data, lvl, checksum=True),
             "stream": lambda: z.compress_stream(data, lvl), "stream4000": lambda: z.compress_stream(data, lvl, 4000)}[how]()
        if how.startswith("stream"):
            assert zc.stats(s)[1]["window_desc"] == 1, name
        n, st = zc.stats(s)
        assert n == len(data), (name, n)
        got, out = zc.decode(s, len(data))
        assert out == data, name
        for m in zc.REQUIRED_MODES:
            if st[m]:
                reached.setdefault(m, name)
        with open(os.path.join(zc.GOLDEN, name + ".zst"), "wb") as f:
            f.write(s)
        e = {"name": name, "file": name + ".zst", "input": key, "libzstd": z.version, "level": lvl, "api": how, "length": len(data), "sha256": zc.sha(data)}
        if len(data) < 4096:
            e["payload_hex"] = data.hex()
        streams.append(e)
        print(f"{name:28s} {len(s):7d} bytes  " + " ".join(k for k in zc.REQUIRED_MODES if st[k]))
    missing = [m for m in zc.REQUIRED_MODES if m not in reached]
    assert not missing, f"no stream reaches {missing}"
    hand = []                                                       # the hand-built frames of zstd_cases.hand_frames(), for the sanitizer program
    for name, (f, exp, host_only) in zc.hand_frames().items():
        with open(os.path.join(zc.GOLDEN, f"hand_{name}.zst"), "wb") as fh:
            fh.write(f)
        hand.append({"name": name, "file": f"hand_{name}.zst", "length": -1 if exp is None else len(exp), "sha256": "" if exp is None else zc.sha(exp),
                     "host_only": host_only})
    files = []
    for name, (arr, opts) in file_rasters().items():
        path = os.path.join(zc.GOLDEN, name + ".tif")
        write_geotiff(path, arr, (0.2, 0, 500000.0, 0, -0.2, 5600000.0), compression="zstd", zstd_level=9, **opts)
        with GeoTiff(path) as g:
            px = g.read()
        assert np.array_equal(px, arr if arr.ndim == 3 else arr[None])
        hwc = np.ascontiguousarray((arr if arr.ndim == 3 else arr[None]).transpose(1, 2, 0))
        files.append({"name": name, "file": name + ".tif", "shape": list(hwc.shape), "dtype": str(hwc.dtype), "pixel_sha256": zc.sha(hwc.tobytes())})
    from PIL import Image
    rgb = np.ascontiguousarray(file_rasters()["rgb_tiles_p2"][0].transpose(1, 2, 0))
    path = os.path.join(zc.GOLDEN, "rgb_pillow.tif")
    Image.fromarray(rgb).save(path, compression="zstd")
    files.append({"name": "rgb_pillow", "file": "rgb_pillow.tif", "shape": list(rgb.shape), "dtype": "uint8", "pixel_sha256": zc.sha(rgb.tobytes())})
    with open(os.path.join(zc.GOLDEN, "manifest.json"), "w") as f:
        json.dump({"streams": streams, "hand": hand, "files": files, "reached_by": reached}, f, indent=1)
    sizes = {f: os.path.getsize(os.path.join(zc.GOLDEN, f)) for f in os.listdir(zc.GOLDEN)}
    assert max(sizes.values()) <= FILE_MAX, max(sizes.items(), key=lambda t: t[1])
    assert all(v < 100 << 10 for k, v in sizes.items() if k.endswith(".tif")), sizes
    assert sum(sizes.values()) < DIR_MAX, sum(sizes.values())
    print(f"{len(streams)} streams, {len(files)} files, {sum(sizes.values())} bytes; every mode reached: {reached}")


if __name__ == "__main__":
    main()
