"""Decode rate of LZW / DEFLATE / JPEG rasters on the GPU (tiffdecode.hip, jpegdecode.hip): python tools/raster_decode_bench.py
[codec=lzw|deflate|jpeg|zstd [level=9]] [side=9000] [tile=256|strip=N] [predictor=2] [data=tiles|noise|flat]
JPEG (predictor ignored): [bands=3 | 4 (RGB + near-infrared: four components as stored, subsampling ignored) | 1] [quality=90] [subsampling=2 (4:2:0) | 1 (4:2:2) | 0 (4:4:4)] [layout=complete|gdal] [restart=MCUs]
[long=1 [subseq=256] [threshold=32768]: a raster with entropy-coded segments above GeoTiff.JPEG_DEVICE_MAX_SEGMENT (no restart markers),
which otherwise "stays with the host reader", is decoded on the device with a wave per long segment (decode_to_device(long_segments=True));
the line then carries the long segments, the walk rounds per window of 64 subsequences (mean, the most, windows of one round) and the
subsequence size] [host_threads=16] — also times the host reader (Pillow's libjpeg per block, on that many threads) on the same raster and checks that
both give the same bytes.
Raster side x side x 4 uint8 (default 9000: the 400 windows of 450 x 450 px the reference cuts from one image, twice over); prints per
call file → pinned → device → decoded raster in HBM, and the kernels alone (HIP events). Under rocprofv3 --kernel-trace --stats the
per-kernel durations land in profiles/r06_decode_kernel_stats.csv.
DEFLATE: the blocks' Adler-32 check is a launch of its own behind the inflate kernel; "inflate_ms" and "checksum_ms" time the two
separately (HIP events around td_tiff_inflate_dev and around td_tiff_adler32_blocks_dev, the raster's blocks already on the device).
samples=f32 [codec=deflate|lzw|zstd [level=9]] [side=9000] [tile=256|strip=N] [predictors=1,2,3]: the float32 height raster of the post-processing
stage (a synthetic nDSM, one band) — per predictor one JSON line with the compressed size, the block decoder's launch and the scatter /
predictor kernel apart (HIP events on the stream they ran on, median of 7 warm runs; the scatter's GB/s counts one read and one
write of the raster), the wall time from the file to a raster td_crown_stats can read for the device path (decode_to_device +
check()) and for the host paths: the block reader (read()) + the copy to the device, and — predictor 3 — the whole image through Pillow
+ the copy, which is how the reader served such files before it undid the floating-point predictor itself.
planar=1 [path=device|host|chunky] [bands=0,3] [codec=lzw|deflate|zstd [level=9]] [side=9000] [tile=256|strip=N] [predictor=2] [host_threads=16]
[file=PATH]: the four-band uint8 raster written band-separate (PlanarConfiguration = 2) — one JSON line for ONE path, so that each runs
in a process of its own: "device" = decode_to_device(planar=True[, bands=...]) from the file to the raster in HBM (wall, best and
median of 5 after a warm-up), then the block decoder's launch and the layout launch (td_tiff_planes_to_image_dev) apart, HIP events,
median of 7 warm runs; "host" = the same file through the host reader on host_threads threads + the copy to the device (what the file
costs with ``device_decode_planar`` off); "chunky" = the same pixels pixel-interleaved on the existing device path, its decoder and
tiff_blocks_to_image_rgbi_kernel apart. ``bands`` (device only) decodes a plane subset, e.g. 0,3 for NDVI. ``file``: the raster is
written there unless it exists, and stays (several paths over one file)."""
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from treedetection_amd import _lib                                  # noqa: E402
from treedetection_amd.device_decode import alloc_block_buffers, launch_block_decoder, launch_layout, stage_offsets      # noqa: E402
from treedetection_amd.geotiff import GeoTiff, write_geotiff      # noqa: E402
from treedetection_amd.synth import make_tile                      # noqa: E402

args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)


def timed(fn, reps=7, warmup=1):
    """HIP events around ``fn()`` on the current stream: ms of ``reps`` runs after ``warmup`` runs that do not count."""
    out = []
    for _ in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out[warmup:]


def staged(g, bands=None):
    """The raster's compressed blocks on the device as decode_to_device stages them (device_block_plan + stage_offsets), the buffers its
    launches write, and decode(verified=True) / layout(image): its two launches on the current stream, to be timed apart.
    → a record of comp, meta, bufs, cap, nb, planes, decode, layout"""
    planes, mask, offs, cnts, expect, ranges = g.device_block_plan(bands)
    rel, starts, span = stage_offsets(offs, ranges)
    comp = torch.zeros((span + 16,), dtype=torch.uint8)
    for s0, (lo, hi) in zip(starts, ranges):
        comp[int(s0):int(s0) + hi - lo] = torch.from_numpy(np.fromfile(g.path, dtype=np.uint8, count=hi - lo, offset=lo))
    comp, meta = comp.cuda(), torch.from_numpy(np.stack([rel, cnts])).cuda()
    cap = g._bw * g._bh * (g.count if g.planar == 1 else 1) * g.dtype.itemsize
    bufs = alloc_block_buffers(g.compression, len(offs), cap, "cuda")
    sp = _lib.stream_ptr()

    def decode(verified=True):
        launch_block_decoder(g.compression, comp, meta, bufs, sp, verified)

    def layout(image):
        launch_layout(bufs.blocks, cap, g._bw, g._bh, g._nx, g._ny, g.count, g._predictor, image, g.width, g.height, sp,
                      mask if g.planar == 2 else None)
    return SimpleNamespace(comp=comp, meta=meta, bufs=bufs, cap=cap, nb=len(offs), planes=planes, decode=decode, layout=layout)


def f32_main():
    from concurrent.futures import ThreadPoolExecutor
    from statistics import median
    side, codec = int(args.get("side", 9000)), args.get("codec", "deflate")
    kw = {"rows_per_strip": int(args["strip"])} if "strip" in args else {"tile": (int(args.get("tile", 256)),) * 2}
    n = -(-side // 1000)
    tiles = [make_tile(i, 1000)[1] for i in range(min(16, n * n))]
    img = np.ascontiguousarray(np.block([[tiles[(r * n + c) % len(tiles)] for c in range(n)] for r in range(n)])[None, :side, :side])
    base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(base, f"td_f32bench_{os.getpid()}.tif")
    pinned, pool = [None], ThreadPoolExecutor(max_workers=8)

    def wall(fn, reps=5):
        out = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out[1:]

    if codec == "zstd":
        kw["zstd_level"] = int(args.get("level", 9))
    for pred in [int(v) for v in args.get("predictors", "1,2,3").split(",")]:
        try:
            write_geotiff(path, img, (1.0, 0, 412000.0, 0, -1.0, 5318000.0 + side), 25832, compression=codec, predictor=pred, **kw)
            g = GeoTiff(path)
            assert g.device_decodable(float_samples=True)

            def device_path():
                image, check = g.decode_to_device("cuda:0", None, pinned, pool)
                return check()
            got = device_path()
            assert np.array_equal(got.cpu().numpy()[:, :, 0].view(np.uint32), img[0].view(np.uint32)), "decoded raster differs from what was written"
            del got
            device_ms = wall(device_path)

            def host_blocks():
                h = GeoTiff(path)
                torch.from_numpy(np.ascontiguousarray(h.read()[0], dtype=np.float32)).to("cuda:0")
                h.close()

            def host_pillow():
                from PIL import Image
                Image.MAX_IMAGE_PIXELS = None
                torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(path)), dtype=np.float32)).to("cuda:0")
            host_ms = wall(host_blocks, 3)
            pillow_ms = wall(host_pillow, 3) if pred == 3 else None
            # the two launches apart, the raster's compressed blocks already on the device
            dev, nb = staged(g), g._nx * g._ny
            image = torch.empty((side, side), dtype=torch.float32, device="cuda")
            plain_ms = timed(lambda: dev.decode(verified=False)) if codec == "deflate" else None
            decode_ms = timed(dev.decode)
            assert int((dev.bufs.status[:nb] != 0).sum()) == 0
            scatter_ms = timed(lambda: dev.layout(image))
            assert np.array_equal(image.cpu().numpy().view(np.uint32), img[0].view(np.uint32))
            raw = img.nbytes
            r3 = lambda v: None if v is None else [round(t, 3) for t in v]
            print(json.dumps({"samples": "f32", "codec": codec, "raster": f"{side}x{side}x1", "layout": kw, "predictor": pred, "blocks": nb,
                              "raw_mb": raw / 1e6, "file_mb": os.path.getsize(path) / 1e6,
                              {"lzw": "lzw_ms", "zstd": "zstd_ms"}.get(codec, "inflate_ms"): r3(plain_ms if plain_ms is not None else decode_ms),
                              "inflate_verified_ms": r3(decode_ms) if plain_ms is not None else None,
                              "scatter_ms": r3(scatter_ms), "scatter_median_ms": round(median(scatter_ms), 3),
                              "scatter_gb_per_s_read_plus_write": 2 * raw / (median(scatter_ms) * 1e-3) / 1e9,
                              "decoder_median_ms": round(median(plain_ms if plain_ms is not None else decode_ms), 3),
                              "device_path_wall_ms": r3(device_ms), "device_path_median_ms": round(median(device_ms), 1),
                              "host_block_reader_plus_h2d_ms": r3(host_ms), "host_block_reader_median_ms": round(median(host_ms), 1),
                              "host_pillow_whole_image_plus_h2d_ms": r3(pillow_ms),
                              "host_pillow_median_ms": None if pillow_ms is None else round(median(pillow_ms), 1)}), flush=True)
            g.close()
            del dev, image
        finally:
            if os.path.exists(path):
                os.unlink(path)


def planar_main():
    from concurrent.futures import ThreadPoolExecutor
    from statistics import median
    side, pred, codec, which = int(args.get("side", 9000)), int(args.get("predictor", 2)), args.get("codec", "lzw"), args.get("path", "device")
    bands = tuple(int(v) for v in args["bands"].split(",")) if "bands" in args else None
    assert which in ("device", "host", "chunky") and (bands is None or which == "device")
    kw = {"rows_per_strip": int(args["strip"])} if "strip" in args else {"tile": (int(args.get("tile", 256)),) * 2}
    if codec == "zstd":
        kw["zstd_level"] = int(args.get("level", 9))
    n = -(-side // 1000)
    tiles = [make_tile(i, 1000)[0] for i in range(min(16, n * n))]
    img = np.zeros((4, n * 1000, n * 1000), np.uint8)
    for r in range(n):
        for c in range(n):
            t = tiles[(r * n + c) % len(tiles)]
            img[:3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t.transpose(2, 0, 1)
            img[3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t[..., 1]
    img = np.ascontiguousarray(img[:, :side, :side])
    base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = args.get("file", os.path.join(base, f"td_planarbench_{os.getpid()}.tif"))
    planar = which != "chunky"
    try:
        if not ("file" in args and os.path.exists(path)):
            write_geotiff(path, img, (0.2, 0, 412000.0, 0, -0.2, 5318000.0 + side * 0.2), 25832, compression=codec, predictor=pred, planar=planar, **kw)
        g = GeoTiff(path)
        assert g.planar == (2 if planar else 1) and g.device_decodable(planar=planar) and not (planar and g.device_decodable())
        want = img.transpose(1, 2, 0).copy()
        if bands is not None:
            want[:, :, [c for c in range(4) if c not in bands]] = 0
        line = {"path": which, "codec": codec, "raster": f"{side}x{side}x4", "layout": kw, "predictor": pred, "planar": planar, "bands": bands,
                "raw_mb": img.nbytes / 1e6, "file_mb": os.path.getsize(path) / 1e6}
        r3 = lambda v: [round(t, 3) for t in v]
        if which == "host":
            nth = int(args.get("host_threads", 16))
            host_ms = []
            for k in range(4):
                h = GeoTiff(path)
                h._setup_blocks()
                keys = [(p, by, bx) for p in range(4) for by in range(h._ny) for bx in range(h._nx)]
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=nth) as hp:
                    blks = list(hp.map(lambda key: h._decode_block(*key), keys))
                ref = np.empty((side, side, 4), np.uint8)
                for (p, by, bx), blk in zip(keys, blks):
                    r0, c0 = by * h._bh, bx * h._bw
                    piece = blk[:min(blk.shape[0], side - r0), :min(h._bw, side - c0), 0]
                    ref[r0:r0 + piece.shape[0], c0:c0 + piece.shape[1], p] = piece
                dev_ref = torch.from_numpy(ref).cuda()
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
                if k == 0:
                    assert np.array_equal(ref, want), "host reader differs from what was written"
                del blks, dev_ref
                h.close()
            line.update(host_threads=nth, host_reader_plus_stitch_plus_h2d_ms=r3(host_ms), host_median_ms=round(median(host_ms[1:]), 1))
            print(json.dumps(line), flush=True)
            return
        pinned, pool = [None], ThreadPoolExecutor(max_workers=8)
        dkw = {"planar": True, "bands": bands} if planar else {}
        wall_ms, kernel_ms = [], []
        for k in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            image, check = g.decode_to_device("cuda:0", None, pinned, pool, **dkw)
            got = check()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            kernel_ms.append(check.kernel_ms)
            if k == 0:
                assert np.array_equal(got.cpu().numpy(), want), "decoded raster differs from what was written"
            del image, got
        line.update(copied_mb=check.compressed_bytes / 1e6, file_to_hbm_ms=r3(wall_ms), file_to_hbm_median_ms=round(median(wall_ms[1:]), 1),
                    file_to_hbm_best_ms=round(min(wall_ms[1:]), 1), both_launches_ms=r3(kernel_ms))
        # the two launches apart, the selected planes' compressed blocks already on the device
        dev = staged(g, bands)
        nb, planes = dev.nb, dev.planes
        image = torch.empty((side, side, 4), dtype=torch.uint8, device="cuda")
        decode_ms = timed(dev.decode)
        assert int((dev.bufs.status[:nb] != 0).sum()) == 0
        layout_ms = timed(lambda: dev.layout(image))
        assert np.array_equal(image.cpu().numpy(), want)
        moved = img.nbytes + len(planes) * (img.nbytes // 4 if planar else img.nbytes)      # one write of the raster + one read of what was decoded
        line.update(blocks=nb, decoder_ms=r3(decode_ms), decoder_median_ms=round(median(decode_ms), 3), layout_ms=r3(layout_ms),
                    layout_median_ms=round(median(layout_ms), 3), layout_gb_per_s_read_plus_write=moved / (median(layout_ms) * 1e-3) / 1e9)
        print(json.dumps(line), flush=True)
    finally:
        if "file" not in args and os.path.exists(path):
            os.unlink(path)


if args.get("samples") == "f32":
    f32_main()
    sys.exit(0)
if args.get("planar") == "1":
    planar_main()
    sys.exit(0)
side, pred, data, codec = int(args.get("side", 9000)), int(args.get("predictor", 2)), args.get("data", "tiles"), args.get("codec", "lzw")
kw = {"rows_per_strip": int(args["strip"])} if "strip" in args else {"tile": (int(args.get("tile", 256)),) * 2}
base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
path = os.path.join(base, f"td_lzwbench_{os.getpid()}.tif")
rng = np.random.default_rng(0)
if data == "noise":
    img = rng.integers(0, 256, (4, side, side), dtype=np.uint8)
elif data == "flat":
    img = np.full((4, side, side), 77, np.uint8)
else:
    n = -(-side // 1000)
    tiles = [make_tile(i, 1000)[0] for i in range(min(16, n * n))]
    img = np.zeros((4, n * 1000, n * 1000), np.uint8)
    for r in range(n):
        for c in range(n):
            t = tiles[(r * n + c) % len(tiles)]
            img[:3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t.transpose(2, 0, 1)
            img[3, r * 1000:(r + 1) * 1000, c * 1000:(c + 1) * 1000] = t[..., 1]
    img = np.ascontiguousarray(img[:, :side, :side])
if codec == "zstd":
    kw["zstd_level"] = int(args.get("level", 9))
if codec == "jpeg":
    img, pred = np.ascontiguousarray(img[:int(args.get("bands", 3))]), 1
    kw.update(jpeg_quality=int(args.get("quality", 90)), jpeg_subsampling=int(args.get("subsampling", 2)),
              jpeg_tables=args.get("layout", "complete") == "gdal", jpeg_restart=int(args.get("restart", 0)))
try:
    t0 = time.perf_counter()
    write_geotiff(path, img, (0.2, 0, 412000.0, 0, -0.2, 5318000.0 + side * 0.2), 25832, compression=codec, predictor=pred, **kw)
    t_enc = time.perf_counter() - t0
    g = GeoTiff(path)
    g._setup_blocks()
    times, ktimes = [], []
    from concurrent.futures import ThreadPoolExecutor
    pinned, pool = [None], ThreadPoolExecutor(max_workers=8)
    # a JPEG raster the device decoder does not take (a segment above GeoTiff.JPEG_DEVICE_MAX_SEGMENT: one lane would walk it alone)
    # stays with the host reader under every setting: only the host reader is timed, and the line says so
    long_kw = {}
    if codec == "jpeg" and args.get("long", "0") == "1":
        long_kw = {"long_segments": True, "subseq_bytes": int(args.get("subseq", GeoTiff.JPEG_SYNC_SUBSEQ)),
                   "long_threshold": int(args["threshold"]) if "threshold" in args else None}
    on_device = codec != "jpeg" or g.device_decodable(long_segments=bool(long_kw))
    sync = {}
    dev0 = slow = None
    for k in range(5 if on_device else 0):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        image, check = g.decode_to_device("cuda:0", None, pinned, pool, **long_kw)
        got = check()
        times.append(time.perf_counter() - t0)
        if long_kw:
            st = check.sync_stats
            sync = {"long_segments": check.long_segments, "subseq_bytes": long_kw["subseq_bytes"], "windows": st[1],
                    "rounds_per_window": round(check.sync_rounds, 2), "most_rounds_of_a_window": st[2], "windows_of_one_round": st[3]}
        ktimes.append(check.kernel_ms)
        slow = getattr(check, "slow_codes", 0)
        if k == 0 and codec == "jpeg":
            dev0 = got.cpu().numpy()
        elif k == 0:
            assert np.array_equal(got.cpu().numpy().transpose(2, 0, 1), img), "decoded raster differs from what was written"
        del image, got
    extra = {}
    if codec == "deflate":
        # the two launches of td_tiff_inflate_verified_dev apart: the decoder alone, then the checksum launch alone over its output
        dev = staged(g)
        bufs, meta, nb, lib, sp = dev.bufs, dev.meta, dev.nb, _lib.load(), _lib.stream_ptr()
        dev.decode()
        assert int((bufs.status[:nb] != 0).sum()) == 0, "a block failed its checksum"
        inflate_ms = timed(lambda: dev.decode(verified=False), 5, 0)
        verified_ms = timed(dev.decode, 5, 0)
        checksum_ms = timed(lambda: _lib.check(lib.td_tiff_adler32_blocks_dev(bufs.blocks.data_ptr(), dev.cap, bufs.decoded.data_ptr(), dev.comp.data_ptr(),
                                                                              meta[0].data_ptr(), meta[1].data_ptr(), bufs.ends.data_ptr(), nb,
                                                                              bufs.status.data_ptr(), sp), "td_tiff_adler32_blocks_dev"), 5, 0)
        assert int((bufs.status[:nb] != 0).sum()) == 0
        extra = {"inflate_ms": [round(t, 3) for t in inflate_ms], "inflate_verified_ms": [round(t, 3) for t in verified_ms],
                 "checksum_ms": [round(t, 3) for t in checksum_ms], "checksum_share_of_inflate": min(checksum_ms) / min(inflate_ms)}
        del dev, bufs, meta
    if codec == "zstd":
        # the launches apart (the decoder, the scatter / predictor kernel), the host reader on host_threads threads (every block through
        # GeoTiff._decode_block: td_tiff_zstd_decode + the predictor), and — once — the whole file through Pillow: how such a file was read before
        dev = staged(g)
        image = torch.empty((g.height, g.width, g.count), dtype=torch.uint8, device="cuda")
        zstd_ms = timed(dev.decode, 5, 0)
        assert int((dev.bufs.status[:dev.nb] != 0).sum()) == 0
        scatter_ms = timed(lambda: dev.layout(image), 5, 0)
        assert np.array_equal(image.cpu().numpy().transpose(2, 0, 1), img)
        del dev, image
        nth = int(args.get("host_threads", 16))
        keys = [(0, by, bx) for by in range(g._ny) for bx in range(g._nx)]
        host_s, host_decode_s = [], []                             # blocks + stitch + copy / the blocks alone: what the JPEG branch times
        for k in range(3):
            h = GeoTiff(path)
            h._setup_blocks()
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=nth) as hp:
                blks = list(hp.map(lambda key: h._decode_block(*key), keys))
            host_decode_s.append(time.perf_counter() - t0)
            ref = np.empty((side, side, img.shape[0]), np.uint8)
            for (_, by, bx), blk in zip(keys, blks):
                r0, c0 = by * h._bh, bx * h._bw
                piece = blk[:min(blk.shape[0], side - r0), :min(h._bw, side - c0)]
                ref[r0:r0 + piece.shape[0], c0:c0 + piece.shape[1]] = piece
            dev_ref = torch.from_numpy(ref).cuda()
            torch.cuda.synchronize()
            host_s.append(time.perf_counter() - t0)
            if k == 0:
                assert np.array_equal(ref.transpose(2, 0, 1), img), "host reader differs from what was written"
            del blks, dev_ref
            h.close()
        pillow_s = None
        if args.get("pillow", "1") == "1":
            from PIL import Image
            Image.MAX_IMAGE_PIXELS = None
            t0 = time.perf_counter()
            try:
                arr = np.asarray(Image.open(path))
                torch.from_numpy(np.ascontiguousarray(arr)).cuda()
                torch.cuda.synchronize()
                pillow_s = time.perf_counter() - t0
            except Exception as e:                                  # (whether Pillow's TIFF plugin opens the layout at all)
                pillow_s = f"failed: {e}"
        extra = {"level": kw["zstd_level"], "zstd_decode_ms": [round(t, 3) for t in zstd_ms], "scatter_ms": [round(t, 3) for t in scatter_ms],
                 "host_threads": nth, "host_reader_ms": [round(t * 1e3, 1) for t in host_decode_s],
                 "host_reader_plus_stitch_plus_h2d_ms": [round(t * 1e3, 1) for t in host_s],
                 "pillow_whole_file_plus_h2d_ms": round(pillow_s * 1e3, 1) if isinstance(pillow_s, float) else pillow_s}
    if codec == "jpeg":
        # the host reader on the same raster: every block through GeoTiff._decode_block (Pillow's libjpeg) on host_threads threads
        nth = int(args.get("host_threads", 16))
        keys = [(0, by, bx) for by in range(g._ny) for bx in range(g._nx)]
        host_s = []
        for k in range(2):
            h = GeoTiff(path)
            h._setup_blocks()
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=nth) as hp:
                blks = list(hp.map(lambda key: h._decode_block(*key), keys))
            host_s.append(time.perf_counter() - t0)
            if k == 0:
                ref = np.empty((side, side, img.shape[0]), np.uint8)
                for (_, by, bx), blk in zip(keys, blks):
                    r0, c0 = by * h._bh, bx * h._bw
                    piece = blk[:min(blk.shape[0], side - r0), :min(h._bw, side - c0)]
                    ref[r0:r0 + piece.shape[0], c0:c0 + piece.shape[1]] = piece
                assert dev0 is None or np.array_equal(ref, dev0), "device decode differs from the host reader"
            del blks
            h.close()
        info, segs, sets, ncoef = g._jpeg_plan()                # (the plan stands whether or not the segment rule admits the raster)
        extra = {"quality": kw["jpeg_quality"], "subsampling": kw["jpeg_subsampling"], "layout": args.get("layout", "complete"),
                 "restart": kw["jpeg_restart"], "segments": len(segs), "table_sets": len(sets), "host_threads": nth,
                 "host_reader_ms": [round(t * 1e3, 1) for t in host_s], "device_equals_host_reader": True if on_device else None,
                 "device_decodable": on_device, "largest_segment_bytes": int(segs[:, 1].max()),
                 "decodable_without_long": g.device_decodable(), **sync}
        kw = {k: v for k, v in kw.items() if not k.startswith("jpeg_")}
    raw = img.nbytes
    if not on_device:
        print(json.dumps({**extra, "codec": codec, "raster": f"{side}x{side}x{img.shape[0]}", "layout": kw, "blocks": g._nx * g._ny, "raw_mb": raw / 1e6,
                          "file_mb": os.path.getsize(path) / 1e6, "encode_s": round(t_enc, 2)}))
        sys.exit(0)
    best = min(times[1:])
    print(json.dumps({**extra, "codec": codec, "raster": f"{side}x{side}x{img.shape[0]}", "layout": kw, "predictor": pred, "data": data, "blocks": g._nx * g._ny, "raw_mb": raw / 1e6,
                      "file_mb": os.path.getsize(path) / 1e6, "ratio": raw / os.path.getsize(path), "encode_s": round(t_enc, 2),
                      "decode_ms": [round(t * 1e3, 1) for t in times], "kernel_ms": [round(t, 1) for t in ktimes],
                      "kernel_gb_per_s": raw / (min(ktimes) * 1e-3) / 1e9, "strings_through_memory": slow, "decode_gb_per_s": raw / best / 1e9,
                      "windows_450x450x4_per_s": raw / best / (450 * 450 * 4)}))
finally:
    os.unlink(path)
