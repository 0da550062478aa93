"""GeoTIFF reader / writer for the tile loader of the prediction stage.

The reference reads rasters through rasterio/GDAL (``rasterio.open`` + ``rasterio.mask.mask(img, shapes, crop=True)``,
TreeDetection/prediction.py:61,164); neither is installed here. The tile loader needs windowed reads of classic or
BigTIFF rasters — strips or tiles, pixel-interleaved or planar, 8/16/32-bit integer or float samples, uncompressed or
DEFLATE (zlib) / LZW / ZSTD / PackBits (td_tiff_*_decode in libtreedet_hip.so), horizontal-differencing predictor — plus the
three geo tags (ModelPixelScale / ModelTiepoint / GeoKeyDirectory). JPEG-in-TIFF (compression 7, 8-bit, one, three or four bands —
RGB + near-infrared as GDAL writes it: RGB with one extra sample, four components stored as they are)
is windowed too: a block's abbreviated stream + the JPEGTables tag form one JPEG stream, decoded by Pillow's libjpeg block by
block (GDAL does the same through libtiff). The floating-point predictor (predictor 3, TIFF Technical Note 3) of float32 rasters
is undone block by block (td_tiff_unpredict_float). Other codecs (old-style JPEG, predictor 3 on float64, ...): whole image through Pillow.
Whole rasters can instead be decoded on the GPU and kept in HBM (``decode_to_device``): LZW, DEFLATE and ZSTD (tiffdecode.hip, zstddecode.hip; uint8 and
native-order uint16 samples; native-order float32 height rasters, predictors 1 - 3, for callers that ask for them) and sequential-Huffman
JPEG (jpegdecode.hip, byte-identical to the Pillow path) — see ``device_decodable`` — or, with ``window=``, only the blocks a pixel window
overlaps (the seam strips of merging.py). The steps of the device paths (staging, the file
read, the decoder and layout launches, ``check``) are device_decode.py's; the methods here compose them.
"""
from __future__ import annotations

import contextlib
import math
import os
import struct
import threading
import zlib
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .device_decode import alloc_block_buffers, finish, launch_block_decoder, launch_layout, read_ranges, stage_offsets

_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2),
          9: ("i", 4), 10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
_DTYPES = {(1, 8): np.uint8, (1, 16): np.uint16, (1, 32): np.uint32, (2, 8): np.int8, (2, 16): np.int16,
           (2, 32): np.int32, (3, 32): np.float32, (3, 64): np.float64}


class GeoTiff:
    """Read-only view of one raster. Arrays come back as [bands, rows, cols] like rasterio's ``read``."""

    def __init__(self, path: str):
        self.path = path
        self._pil = None
        with open(path, "rb") as f:
            head = f.read(16)
            if head[:2] == b"II":
                self._e = "<"
            elif head[:2] == b"MM":
                self._e = ">"
            else:
                raise ValueError(f"{path}: not a TIFF")
            magic = struct.unpack(self._e + "H", head[2:4])[0]
            self._big = magic == 43
            if magic not in (42, 43):
                raise ValueError(f"{path}: bad TIFF magic {magic}")
            if self._big:
                ifd = struct.unpack(self._e + "Q", head[8:16])[0]
            else:
                ifd = struct.unpack(self._e + "I", head[4:8])[0]
            self.tags = self._read_ifd(f, ifd)
        t = self.tags
        self.width = int(t[256][0])
        self.height = int(t[257][0])
        self.count = int(t.get(277, [1])[0])
        bits = int(t.get(258, [8])[0])
        fmt = int(t.get(339, [1])[0])
        if (fmt, bits) not in _DTYPES:
            raise ValueError(f"{path}: unsupported sample format {fmt}/{bits} bits")
        self.dtype = np.dtype(_DTYPES[(fmt, bits)]).newbyteorder(self._e)
        self.planar = int(t.get(284, [1])[0])
        self.compression = int(t.get(259, [1])[0])
        self._data: Optional[np.ndarray] = None
        # georeferencing
        if 33550 in t and 33922 in t:
            sx, sy = float(t[33550][0]), float(t[33550][1])
            i, j, _, x, y, _ = (float(v) for v in t[33922][:6])
            self.transform = (sx, 0.0, x - i * sx, 0.0, -sy, y + j * sy)
        elif 34264 in t:
            m = [float(v) for v in t[34264]]
            self.transform = (m[0], m[1], m[3], m[4], m[5], m[7])
        else:
            self.transform = (1.0, 0.0, 0.0, 0.0, -1.0, float(self.height))
        # GDAL_NODATA (tag 42113, ASCII): what rasterio reports as ``src.nodata`` (helpers.merge_images reads it)
        self.nodata: Optional[float] = None
        if 42113 in t:
            try:
                self.nodata = float(str(t[42113][0]).strip())
            except (ValueError, IndexError):
                self.nodata = None
        self.epsg = None
        if 34735 in t:
            keys = [int(v) for v in t[34735]]
            for k in range(4, len(keys) - 3, 4):
                if keys[k] in (3072, 2048) and keys[k + 1] == 0:
                    self.epsg = keys[k + 3]
                    if keys[k] == 3072:
                        break

    # -- tiff structure ---------------------------------------------------------------------------
    def _read_ifd(self, f, off) -> Dict[int, Sequence]:
        e = self._e
        f.seek(off)
        if self._big:
            n = struct.unpack(e + "Q", f.read(8))[0]
            ent, fmt, inl = 20, e + "HHQ", 8
        else:
            n = struct.unpack(e + "H", f.read(2))[0]
            ent, fmt, inl = 12, e + "HHI", 4
        raw = f.read(n * ent)
        tags = {}
        for i in range(n):
            rec = raw[i * ent:(i + 1) * ent]
            tag, typ, cnt = struct.unpack(fmt, rec[:ent - inl])
            if typ not in _TYPES:
                continue
            code, size = _TYPES[typ]
            total = size * cnt
            if total <= inl:
                buf = rec[ent - inl:ent - inl + total]
            else:
                ptr = struct.unpack(e + ("Q" if self._big else "I"), rec[ent - inl:])[0]
                pos = f.tell()
                f.seek(ptr)
                buf = f.read(total)
                f.seek(pos)
            if typ == 2:
                tags[tag] = [buf.rstrip(b"\0").decode("latin1")]
            elif typ in (5, 10):
                v = struct.unpack(e + str(cnt * 2) + code[0], buf)
                tags[tag] = [v[2 * k] / v[2 * k + 1] if v[2 * k + 1] else 0.0 for k in range(cnt)]
            else:
                tags[tag] = list(struct.unpack(e + str(cnt) + code, buf))
        return tags

    # -- pixel access ---------------------------------------------------------------------------------
    # The raster is a grid of blocks (strips = full-width blocks of RowsPerStrip rows; tiles = TileWidth x TileLength),
    # chunky (one block holds all bands, pixel-interleaved) or planar (one grid per band). A window read touches only
    # the blocks it overlaps; decoded blocks of compressed files are kept in a small LRU cache because neighbouring
    # tile windows (buffer overlap) share them. Uncompressed chunky files whose strips are contiguous skip all of
    # this: the window is a slice of one memory map.
    _CACHE_BYTES = 256 << 20

    def _setup_blocks(self) -> None:
        if getattr(self, "_blocks_ready", False):
            return
        t = self.tags
        H, W = self.height, self.width
        if 324 in t:
            self._bw, self._bh = int(t[322][0]), int(t[323][0])
            self._offs, self._counts = [int(v) for v in t[324]], [int(v) for v in t[325]]
            self._strips = False
        else:
            self._bw, self._bh = W, min(int(t.get(278, [H])[0]), H)
            self._offs = [int(v) for v in t[273]]
            self._counts = [int(v) for v in t[279]] if 279 in t else None
            self._strips = True
        self._nx = (W + self._bw - 1) // self._bw
        self._ny = (H + self._bh - 1) // self._bh
        self._predictor = int(t.get(317, [1])[0])
        self._mm = np.memmap(self.path, dtype=np.uint8, mode="r")
        self._cache: "OrderedDict" = OrderedDict()
        self._cache_bytes = 0
        self._lock = threading.Lock()
        self._pool = None
        self._flat = None
        self._fd = None
        item = self.dtype.itemsize
        if self.compression == 1 and self.planar == 1 and self._strips and self._predictor == 1:     # (a predictor is undone per block)
            row_bytes = W * self.count * item
            offs = self._offs
            if all(offs[i + 1] - offs[i] == self._bh * row_bytes for i in range(len(offs) - 1)):
                self._flat = np.memmap(self.path, dtype=self.dtype, mode="r", offset=offs[0], shape=(H, W, self.count))
                if self.dtype.byteorder in ("=", "|") and os.path.getsize(self.path) >= offs[0] + H * row_bytes:
                    # windows are read with pread (td_read_window): no page fault per window row, no munmap of a touched
                    # mapping at close; the map stays for whole-raster reads and foreign byte orders
                    self._fd, self._flat_off = os.open(self.path, os.O_RDONLY), offs[0]
        if self.compression == 7 and self._jpeg_blocks_ok():
            tb = bytes(bytearray(int(v) for v in t.get(347, [])))
            self._jpeg_tables = tb if len(tb) >= 4 and tb[:2] == b"\xff\xd8" and tb[-2:] == b"\xff\xd9" else b""
        elif self.compression not in (1, 5, 8, 32946, 32773, 50000) or not (self._predictor in (1, 2) or self._float_predictor()):
            self._pil_fallback()
        self._blocks_ready = True

    def _float_predictor(self) -> bool:
        """Predictor 3 on float32 samples (either byte order): undone per block by td_tiff_unpredict_float."""
        return self._predictor == 3 and self.dtype.kind == "f" and self.dtype.itemsize == 4

    def _jpeg_blocks_ok(self) -> bool:
        """New-style JPEG blocks this reader decodes one by one: 8-bit chunky samples, grey, three bands (RGB or YCbCr) or four (RGB
        with an extra sample of any kind, or separated: libtiff stores the four components without a colour transform)."""
        if not (self.dtype == np.uint8 and self.planar == 1 and self._predictor == 1):
            return False
        photometric = int(self.tags.get(262, [2 if self.count >= 3 else 1])[0])
        return photometric in (2, 5) if self.count == 4 else self.count in (1, 3) and photometric in (1, 2, 6)

    def _decode_jpeg_block(self, raw: bytes, rows: int) -> np.ndarray:
        """One strip / tile of a compression-7 raster → uint8 [rows, bw, bands]. TIFF Technical Note 2: the block is an abbreviated JPEG
        stream (SOI, frame and scan headers, entropy-coded data, EOI); the quantisation / Huffman tables it leaves out are in the
        JPEGTables tag (SOI, DQT / DHT segments, EOI) — tables minus its EOI + block minus its SOI is a complete stream. The colour
        space is NOT in the stream (no JFIF header): libtiff tells libjpeg from PhotometricInterpretation; here an Adobe APP14 segment
        (transform 0 = as stored, 1 = YCbCr) says the same thing to Pillow's libjpeg. Four bands need none: libjpeg takes four
        components as stored (CMYK), and Pillow's JPEG plugin, which reads CMYK in Adobe's inverted polarity, is told to unpack the
        decoder's bytes as they are — the samples the file stores, which is what libtiff hands out for RGB + extra sample.
        An Adobe segment of the block's own that names a transform (YCCK) is refused: libtiff would not convert it either."""
        import io
        from PIL import Image
        data = bytes(raw)
        if data[:2] != b"\xff\xd8":
            raise ValueError(f"{self.path}: a JPEG block does not start with SOI")
        head = b"\xff\xd8"
        if self.count == 3 and b"JFIF\0" not in data[:32]:
            ycc = int(self.tags.get(262, [2])[0]) == 6
            head += b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + (b"\x01" if ycc else b"\x00")
        stream = head + self._jpeg_tables[2:-2] + data[2:]
        with Image.open(io.BytesIO(stream)) as im:
            if im.format != "JPEG" or im.mode != {1: "L", 3: "RGB", 4: "CMYK"}[self.count]:
                raise ValueError(f"{self.path}: a JPEG block decodes to mode {im.mode}")
            if self.count == 4:
                if im.info.get("adobe_transform", 0) != 0:
                    raise ValueError(f"{self.path}: a four-band JPEG block with Adobe colour transform {im.info['adobe_transform']} (YCCK)")
                im.tile = [(t[0], t[1], t[2], ("CMYK",) + tuple(t[3][1:])) for t in im.tile]     # raw mode CMYK, not "CMYK;I": no inversion
            arr = np.asarray(im)
        arr = arr[:, :, None] if arr.ndim == 2 else arr
        if arr.shape[0] < rows or arr.shape[1] != self._bw or arr.shape[2] != self.count:
            raise ValueError(f"{self.path}: a JPEG block decodes to {arr.shape}, expected at least ({rows}, {self._bw}, {self.count})")
        return arr[:rows]

    def _pil_fallback(self) -> None:
        """Codecs this reader does not implement (old-style JPEG, floating-point predictor on float64, ...): whole image through Pillow."""
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
        arr = np.asarray(Image.open(self.path))
        arr = arr[:, :, None] if arr.ndim == 2 else arr
        if arr.shape[2] != self.count:
            raise ValueError(f"{self.path}: compression {self.compression} / predictor {self._predictor} is not supported "
                             f"for {self.count}-band rasters")
        self._flat = np.ascontiguousarray(arr)

    def close(self) -> None:
        """Releases the decode threads, the block cache and the file mapping (the object can still be re-used: they are
        rebuilt on the next read)."""
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=False)
        self._pool = None
        self._data = None
        self._blocks_ready = False
        fd = getattr(self, "_fd", None)
        if fd is not None:
            self._fd = None
            os.close(fd)
        for name in ("_cache", "_mm", "_flat"):
            if hasattr(self, name):
                setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            pool = getattr(self, "_pool", None)
            if pool is not None:
                pool.shutdown(wait=False)
            fd = getattr(self, "_fd", None)
            if fd is not None:
                self._fd = None
                os.close(fd)
        except Exception:
            pass

    def _block_rows(self, by: int) -> int:
        return min(self._bh, self.height - by * self._bh) if self._strips else self._bh

    def _decode_block(self, plane: int, by: int, bx: int) -> np.ndarray:
        """→ [rows, bw, bands-in-block] in native byte order, predictor undone."""
        idx = (plane * self._ny + by) * self._nx + bx
        rows = self._block_rows(by)
        cb = self.count if self.planar == 1 else 1
        nbytes = rows * self._bw * cb * self.dtype.itemsize
        off = self._offs[idx]
        cnt = self._counts[idx] if self._counts is not None else nbytes
        raw = self._mm[off:off + cnt]
        comp = self.compression
        if comp == 7:
            return self._decode_jpeg_block(raw, rows)
        if comp == 1:
            buf = np.asarray(raw[:nbytes])
        elif comp in (8, 32946):
            buf = np.frombuffer(zlib.decompress(raw), dtype=np.uint8)
        else:
            from . import _lib
            lib = _lib.load()
            src = np.ascontiguousarray(raw)
            buf = np.empty(nbytes, dtype=np.uint8)
            fn = {5: lib.td_tiff_lzw_decode, 50000: lib.td_tiff_zstd_decode}.get(comp, lib.td_tiff_packbits_decode)
            n = fn(src.ctypes.data, src.size, buf.ctypes.data, nbytes)
            if comp == 50000 and n < 0:                    # corrupt, or more than the block's bytes (libtiff would stop reading there: DESIGN.md §7)
                raise ValueError(f"{self.path}: block ({plane},{by},{bx}) does not decode to its {nbytes} bytes: "
                                 f"{lib.td_last_error().decode('utf-8', 'replace')}")
            _lib.check(n, "tiff block decode")
            buf = buf[:n]
        if buf.size < nbytes:
            raise ValueError(f"{self.path}: block ({plane},{by},{bx}) decodes to {buf.size} bytes, expected {nbytes}")
        if self._predictor == 3:                      # defined on the block's BYTES (planes, most significant first, in every file): undone
            from . import _lib                        # before anything reads them as samples; the result is native floats
            raw4 = np.array(buf[:nbytes], dtype=np.uint8)
            _lib.check(_lib.load().td_tiff_unpredict_float(raw4.ctypes.data, rows, self._bw, cb, self.dtype.itemsize), "td_tiff_unpredict_float")
            return raw4.view(np.float32).reshape(rows, self._bw, cb)
        blk = np.frombuffer(buf[:nbytes], dtype=self.dtype).reshape(rows, self._bw, cb)
        if self.dtype.byteorder not in ("=", "|"):     # file byte order differs from the host's
            blk = blk.astype(self.dtype.newbyteorder("="))
        if self._predictor == 2:                      # horizontal differencing per sample, modulo the sample width
            from . import _lib
            if not blk.flags.writeable or not blk.flags.c_contiguous:
                blk = np.array(blk)
            _lib.check(_lib.load().td_tiff_unpredict(blk.ctypes.data, rows, self._bw, cb, blk.dtype.itemsize), "td_tiff_unpredict")
        return blk

    def _get_block(self, key) -> np.ndarray:
        with self._lock:
            blk = self._cache.get(key)
            if blk is not None:
                self._cache.move_to_end(key)
                return blk
        blk = self._decode_block(*key)
        if self.compression != 1 or self._predictor != 1:
            with self._lock:
                if key not in self._cache:
                    self._cache[key] = blk
                    self._cache_bytes += blk.nbytes
                    while self._cache_bytes > self._CACHE_BYTES and len(self._cache) > 1:
                        _, old = self._cache.popitem(last=False)
                        self._cache_bytes -= old.nbytes
        return blk

    def _window_hwc(self, r0: int, c0: int, h: int, w: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Pixels [r0:r0+h, c0:c0+w] of every band as [h, w, bands] (into ``out`` when given)."""
        self._setup_blocks()
        if self._flat is not None and getattr(self, "_fd", None) is not None:
            if out is None:
                out = np.empty((h, w, self.count), dtype=self.dtype)
            if out.flags.c_contiguous and out.dtype == self.dtype:
                from . import _lib
                px = self.count * self.dtype.itemsize
                n = _lib.load().td_read_window(self._fd, self._flat_off + (r0 * self.width + c0) * px, self.width * px, w * px, h,
                                               out.ctypes.data)
                _lib.check(n, "td_read_window")
                return out
        if self._flat is not None:
            src = self._flat[r0:r0 + h, c0:c0 + w, :]
            if out is None:
                return np.ascontiguousarray(src)
            np.copyto(out, src)
            return out
        if out is None:
            out = np.empty((h, w, self.count), dtype=self.dtype.newbyteorder("="))
        by0, by1 = r0 // self._bh, (r0 + h - 1) // self._bh
        bx0, bx1 = c0 // self._bw, (c0 + w - 1) // self._bw
        planes = self.count if self.planar == 2 else 1
        keys = [(p, by, bx) for p in range(planes) for by in range(by0, by1 + 1) for bx in range(bx0, bx1 + 1)]
        if len(keys) > 1 and self.compression != 1:
            if self._pool is None:
                self._pool = ThreadPoolExecutor(max_workers=min(8, max(2, len(os.sched_getaffinity(0)))))
            # zlib / the C decoders release the GIL; a few blocks per task keep the executor overhead small
            per = max(1, (len(keys) + 15) // 16)
            chunks = [keys[i:i + per] for i in range(0, len(keys), per)]
            blocks = [b for part in self._pool.map(lambda ks: [self._get_block(k) for k in ks], chunks) for b in part]
        else:
            blocks = [self._get_block(k) for k in keys]
        for (p, by, bx), blk in zip(keys, blocks):
            br0, bc0 = by * self._bh, bx * self._bw
            rs, re = max(r0, br0), min(r0 + h, br0 + blk.shape[0])
            cs, ce = max(c0, bc0), min(c0 + w, bc0 + self._bw)
            piece = blk[rs - br0:re - br0, cs - bc0:ce - bc0, :]
            if self.planar == 2:
                out[rs - r0:re - r0, cs - c0:ce - c0, p] = piece[:, :, 0]
            else:
                out[rs - r0:re - r0, cs - c0:ce - c0, :] = piece
        return out

    # -- compressed raster → HBM (tiffdecode.hip) --------------------------------------------------------------------------
    def device_decodable(self, float_samples: bool = False, long_segments: bool = False, planar: bool = False) -> bool:
        """True when the raster's blocks can be decoded on the GPU: LZW, DEFLATE (zlib) or ZSTD strips or tiles of pixel-interleaved
        uint8 or native-order (little-endian) uint16 samples (<= 4 per pixel), predictor 1 or 2; JPEG (compression 7) grey,
        three-band or four-band blocks when the host plan (td_tiff_jpeg_plan: sequential Huffman, 8-bit, 4:4:4 / 4:2:2 / 4:2:0, four
        components all 1x1 and stored as they are) accepts every one of them. ``float_samples=True`` (the height raster of the post-processing stage; the tile loop never asks) also admits
        native-order float32 samples in the same LZW / DEFLATE / ZSTD layouts, predictor 1, 2 or 3 (floating-point predictor). Everything
        else keeps the host reader: big-endian files, planar files (unless ``planar=True``, below), PackBits, int16 / int32 and float64 samples, 12-bit JPEG — and JPEG
        rasters with an entropy-coded segment beyond JPEG_DEVICE_MAX_SEGMENT (blocks without restart markers), unless
        ``long_segments=True``: ``decode_to_device(long_segments=True)`` decodes such segments with a whole wave each.
        ``planar=True`` (the ``device_decode_planar`` config key; default off) admits band-separate files (PlanarConfiguration = 2: one
        grid of blocks per band) under otherwise the same rules — LZW / DEFLATE / ZSTD, the same sample types, band counts and
        predictors, a block (one sample per pixel) below 2^31 bytes; ``decode_to_device(planar=True)`` decodes their planes with the
        same decoders and interleaves them in one launch (td_tiff_planes_to_image*_dev). Planar JPEG keeps the host reader."""
        self._setup_blocks()
        if self.compression == 7:
            if not (hasattr(self, "_jpeg_tables") and self._counts is not None and self._pil is None and self._flat is None):
                return False
            plan = self._jpeg_plan()
            return plan is not None and (long_segments or int(plan[1][:, 1].max()) <= self.JPEG_DEVICE_MAX_SEGMENT)
        f32 = float_samples and self.dtype.kind == "f" and self.dtype.itemsize == 4 and self.dtype.isnative
        layout = self.planar == 1 or (bool(planar) and self.planar == 2)
        return (self.compression in (5, 8, 32946, 50000) and layout and (self._device_samples() or f32) and 1 <= self.count <= 4
                and self._predictor in ((1, 2, 3) if f32 else (1, 2)) and self._counts is not None and self._pil is None
                and self._bw * self._bh * (self.count if self.planar == 1 else 1) * self.dtype.itemsize < (1 << 31))

    def _window_blocks(self, window):
        """``window`` = (r0, c0, h, w) in raster pixels, non-empty and inside the raster (ValueError naming it otherwise) → the
        sub-grid of blocks it overlaps, (by0, bx0, ny', nx')."""
        self._setup_blocks()
        try:
            r0, c0, h, w = (int(v) for v in window)
            ok = all(int(v) == v for v in window)
        except (TypeError, ValueError):
            ok = False
        if not ok or h < 1 or w < 1 or r0 < 0 or c0 < 0 or r0 + h > self.height or c0 + w > self.width:
            raise ValueError(f"{self.path}: window {window!r} (r0, c0, h, w) must be non-empty and lie inside the {self.height} x {self.width} raster")
        by0, bx0 = r0 // self._bh, c0 // self._bw
        return by0, bx0, (r0 + h - 1) // self._bh - by0 + 1, (c0 + w - 1) // self._bw - bx0 + 1

    def device_block_plan(self, bands: Optional[Sequence[int]] = None, window: Optional[Sequence[int]] = None):
        """What ``decode_to_device`` reads and decodes, worked out on the host (no GPU): → (planes, plane_mask, offsets, counts, expect,
        ranges), and with ``window`` (below) a seventh entry. A pixel-interleaved file has one "plane" (0) whose blocks hold every band, and ``bands`` is refused. A band-separate
        file has one grid of nx x ny blocks per band: ``bands`` (band indices, any order, default all) picks the planes — ascending in
        ``planes``, bit p of ``plane_mask`` for band p — and only their blocks are listed: ``offsets`` / ``counts`` are the file's
        own (int64, plane after plane, within a plane the file's order), ``expect`` is what each block must decode to in bytes (every
        plane of a strip file ends in its own short strip). ``ranges`` are the byte ranges [(lo, hi), ...] of the file that hold
        those blocks, one per plane, ascending, merged where they overlap or lie within 4 KB of each other: what is read and copied to the device.
        ``window`` = (r0, c0, h, w) in raster pixels (non-empty, inside the raster: ValueError otherwise): only the blocks of the
        sub-grid by0..by1 x bx0..bx1 the window overlaps are listed, per selected plane, row-major — to the layout kernels a small
        raster of its own — and the result ends in that sub-grid, (by0, bx0, ny', nx'). ``ranges`` then hold one span per plane AND
        BLOCK ROW of the sub-grid before the merge within 4 KB, not one per plane: in a tiled file a block row's tiles bx0..bx1 lie
        side by side, but between two block rows lie the tiles left and right of the window — a window one tile wide in a raster 36
        tiles wide would read 36 times its bytes in one range per plane. In a strip file the rows of a plane are adjacent and merge
        back into one range."""
        self._setup_blocks()
        per = self._nx * self._ny
        item = self.dtype.itemsize
        by0, bx0, ny, nx = (0, 0, self._ny, self._nx) if window is None else self._window_blocks(window)
        if self.planar != 2:
            if bands is not None:
                raise ValueError(f"{self.path}: bands={tuple(bands)!r} picks planes of a band-separate file; this one is pixel-interleaved")
            planes, cb = [0], self.count
        else:
            planes, cb = sorted(set(int(b) for b in (range(self.count) if bands is None else bands))), 1
            if not planes or planes[0] < 0 or planes[-1] >= self.count or (bands is not None and len(planes) != len(list(bands))):
                raise ValueError(f"{self.path}: bands={tuple(bands)!r} must be distinct band indices below {self.count}")
        if self._counts is None or len(self._offs) != len(self._counts) or len(self._offs) != per * (self.count if self.planar == 2 else 1):
            raise ValueError(f"{self.path}: {len(self._offs)} block offsets for {per} blocks per plane")
        sub = ((by0 + np.arange(ny))[:, None] * self._nx + bx0 + np.arange(nx)[None, :]).ravel()      # the sub-grid's blocks within a plane
        idx = np.concatenate([p * per + sub for p in planes])
        offs = np.asarray(self._offs, dtype=np.int64)[idx]
        cnts = np.asarray(self._counts, dtype=np.int64)[idx]
        one = np.array([self._block_rows(by) * self._bw * cb * item for by in range(by0, by0 + ny) for _ in range(nx)], dtype=np.int64)
        expect = np.tile(one, len(planes))
        run = ny * nx if window is None else nx                # blocks that share a span: a plane's, or with a window one block row's
        spans = sorted((int(offs[i:i + run].min()), int((offs + cnts)[i:i + run].max())) for i in range(0, len(idx), run))
        ranges = [spans[0]]
        for lo, hi in spans[1:]:
            if lo <= ranges[-1][1] + 4096:                 # (writers pad blocks to even or page offsets: a small gap is read with its neighbours)
                ranges[-1] = (ranges[-1][0], max(ranges[-1][1], hi))
            else:
                ranges.append((lo, hi))
        mask = sum(1 << p for p in planes) if self.planar == 2 else 1
        plan = (planes, mask, offs, cnts, expect, ranges)
        return plan if window is None else plan + ((by0, bx0, ny, nx),)

    def _device_samples(self) -> bool:
        """Sample types the device kernels take as they lie in the file: uint8, and uint16 in the host's (= the GPU's) byte order."""
        return self.dtype == np.uint8 or (self.dtype.kind == "u" and self.dtype.itemsize == 2 and self.dtype.isnative)

    # One lane decodes one entropy-coded segment at ~1.1 MB/s (a 4096² raster in ONE block without restart markers: 4.0 s on the
    # device against 85 ms for the host reader): rasters with a larger segment stay with the host reader
    JPEG_DEVICE_MAX_SEGMENT = 32 << 10
    # ... unless the caller asks for the wave-per-segment decoder (``long_segments=True``), which cuts a longer segment into
    # subsequences of this many bytes, one per lane (td_tiff_jpeg_decode_long_dev; measured in DESIGN.md §7)
    JPEG_SYNC_SUBSEQ = 256

    def _jpeg_plan(self):
        """The JPEG raster's decode plan (td_tiff_jpeg_plan over the blocks as they lie in the file), or None when a block is not one
        the device decoder takes. Computed once: (block_info [nb, 8], segments [nseg, 4] with file offsets, table sets, coefficients)."""
        if getattr(self, "_jpeg_plan_cache", False) is not False:
            return self._jpeg_plan_cache
        from . import _lib
        lib = _lib.load()
        nb = self._nx * self._ny
        offs = np.asarray(self._offs, dtype=np.int64)
        cnts = np.asarray(self._counts, dtype=np.int64)
        plan = None
        if len(offs) == nb == len(cnts) and int((offs + cnts).max()) <= self._mm.size and int(offs.min()) >= 0:
            rows = np.array([self._block_rows(by) for by in range(self._ny) for _ in range(self._nx)], dtype=np.int32)
            tables = np.frombuffer(self._jpeg_tables, dtype=np.uint8) if self._jpeg_tables else np.zeros(1, np.uint8)
            photometric = int(self.tags.get(262, [2 if self.count >= 3 else 1])[0])
            info = np.zeros((nb, 8), dtype=np.int64)
            totals = np.zeros(4, dtype=np.int64)
            segs, sets = np.zeros((nb, 4), dtype=np.int64), np.zeros((4, _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
            for _ in range(2):                                  # the second call with the sizes the first one reported
                st = lib.td_tiff_jpeg_plan(tables.ctypes.data, len(self._jpeg_tables), self._mm.ctypes.data, offs.ctypes.data,
                                           cnts.ctypes.data, nb, photometric, self.count, self._bw, rows.ctypes.data, info.ctypes.data,
                                           segs.ctypes.data, len(segs), sets.ctypes.data, len(sets), totals.ctypes.data)
                if st != _lib.ERR_CAPACITY:
                    break
                segs = np.zeros((int(totals[0]), 4), dtype=np.int64)
                sets = np.zeros((int(totals[1]), _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
            _lib.check(st, "td_tiff_jpeg_plan")
            if totals[3] == 0:
                plan = (info, segs[:int(totals[0])], sets[:int(totals[1])], int(totals[2]))
        self._jpeg_plan_cache = plan
        return plan

    def decode_to_device(self, device, stream=None, pinned=None, pool=None, long_segments: bool = False, long_threshold: Optional[int] = None,
                         subseq_bytes: Optional[int] = None, planar: bool = False, bands: Optional[Sequence[int]] = None,
                         window: Optional[Sequence[int]] = None):
        """The whole raster decoded in HBM: the compressed blocks are read as they lie in the file (one pread of the span that
        holds them, into pinned memory), copied to the device once, decoded one wave per block (td_tiff_lzw_decode_dev / td_tiff_zstd_decode_dev /
        td_tiff_inflate_verified_dev, which also checks every DEFLATE block's Adler-32 trailer as zlib does; JPEG: one lane per
        entropy-coded segment, td_tiff_jpeg_decode_dev, planned once by td_tiff_jpeg_plan) and
        laid out as [height, width, bands] uint8 — or torch.uint16 for 16-bit rasters, torch.float32 for float32 rasters — with
        predictor 2 (float32: or 3) undone (td_tiff_blocks_to_image_dev / td_tiff_blocks_to_image_u16_dev / td_tiff_blocks_to_image_f32_dev). → (image tensor, check) where ``check()`` waits for the kernels and raises ValueError when a block did not decode to its size
        or, DEFLATE, its bytes do not sum to the stream's checksum ("Adler-32 mismatch": the host reader's zlib raises on the same block) — the
        caller then falls back to the host reader. Everything is enqueued on ``stream`` (default: the current one). ``pinned``:
        a one-element list holding a pinned uint8 tensor to read the file into (grown and put back when too small — pinning
        hundreds of MB per image costs as much as reading them); ``pool``: threads the file read is spread over.
        ``long_segments`` (JPEG only): entropy-coded segments of more than ``long_threshold`` bytes (default JPEG_DEVICE_MAX_SEGMENT;
        0: every segment) are decoded by one wave each, in subsequences of ``subseq_bytes`` (default JPEG_SYNC_SUBSEQ), the others one
        per lane as ever (td_tiff_jpeg_decode_long_dev); ``check`` then carries ``.long_segments`` (how many took the wave) and
        ``.sync_rounds`` (walk rounds per window of 64 subsequences, mean; 1.0 = every guess was right).
        ``planar=True`` takes band-separate files too (``device_decodable(planar=True)``): every plane's blocks go through the same
        decoders, one sample per pixel, and td_tiff_planes_to_image_dev / _u16_dev / _f32_dev interleaves them into the same
        [height, width, bands] tensor in one launch. ``bands`` (band-separate files only; ValueError otherwise): the band indices that
        are needed — only their planes are read from the file, copied and decoded (:meth:`device_block_plan`); the image keeps all its
        channels, the others are 0, and ``check.compressed_bytes`` counts what was copied.
        ``window`` = (r0, c0, h, w) in raster pixels (non-empty, inside the raster: ValueError otherwise): only the blocks the window
        overlaps are read, copied and decoded (:meth:`device_block_plan`), and the tensor is their block-aligned COVER
        [cover_h, cover_w, bands], whose pixel (0, 0) is the raster's ``check.origin`` = (by0 * block rows, bx0 * block columns) and
        which ends with the sub-grid or the raster, whichever comes first; the window lies in it at ``check.window`` = (row, column,
        h, w). The same decoder and layout launches on the sub-grid as on a small raster of its own; a bad block is still named by
        its number in the file. JPEG rasters ignore the window: they decode whole, origin (0, 0)."""
        import torch
        from . import _lib
        if not self.device_decodable(float_samples=True, long_segments=long_segments, planar=planar):
            raise ValueError(f"{self.path}: not decodable on the device (compression {self.compression}, {self.dtype}, {self.count} bands)")
        dev = torch.device(device)
        by0, bx0, ny, nx = 0, 0, self._ny, self._nx
        if window is not None and self.compression != 7:
            planes, plane_mask, offs, cnts, expect, ranges, (by0, bx0, ny, nx) = self.device_block_plan(bands, window)
        else:
            if window is not None:
                self._window_blocks(window)                     # (refused like any other raster's when it is bad)
            planes, plane_mask, offs, cnts, expect, ranges = self.device_block_plan(bands)
        oy, ox = by0 * self._bh, bx0 * self._bw
        cover_h, cover_w = min((by0 + ny) * self._bh, self.height) - oy, min((bx0 + nx) * self._bw, self.width) - ox
        where = {} if window is None else {"origin": (oy, ox), "window": (int(window[0]) - oy, int(window[1]) - ox, int(window[2]), int(window[3]))}
        nb = len(offs)
        rel, starts, span = stage_offsets(offs, ranges)
        if pinned is not None and pinned and pinned[0] is not None and pinned[0].numel() >= span + 16:
            pin = pinned[0]
        else:
            pin = torch.empty((span + 16 + (span >> 3),), dtype=torch.uint8, pin_memory=True)
            if pinned is not None:
                pinned[:] = [pin]
        buf = pin.numpy()
        piece = 8 << 20
        parts = [(int(s0) + p, min(piece, r1 - r0 - p), r0 + p) for s0, (r0, r1) in zip(starts, ranges) for p in range(0, r1 - r0, piece)]
        for _ in read_ranges(self.path, parts, buf, pool, "block data"):
            pass
        buf[span:] = 0
        item = self.dtype.itemsize                              # block sizes, capacities and what a block must decode to count BYTES
        block_cap = self._bw * self._bh * (self.count if self.planar == 1 else 1) * item
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with torch.cuda.device(dev), ctx:
            st = _lib.stream_ptr()
            comp = pin[:span + 16].to(dev, non_blocking=True)
            k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if self.compression == 7:
                return self._jpeg_to_device(dev, pin, comp, ranges[0][0], span, k0, k1, long_segments, long_threshold, subseq_bytes, where)
            meta = torch.from_numpy(np.stack([rel, cnts])).to(dev, non_blocking=True)
            bufs = alloc_block_buffers(self.compression, nb, block_cap, dev)
            k0.record()
            launch_block_decoder(self.compression, comp, meta, bufs, st)
            image = torch.empty((cover_h, cover_w, self.count), dtype={1: torch.uint8, 2: torch.uint16, 4: torch.float32}[item], device=dev)
            launch_layout(bufs.blocks, block_cap, self._bw, self._bh, nx, ny, self.count, self._predictor, image, cover_w,
                          cover_h, st, plane_mask if self.planar == 2 else None)
            k1.record()                                    # the decode launches (DEFLATE: + the checksum launch) + the scatter / predictor kernel

            def verdict(check, dec_h, st_h):
                produced = dec_h & 0xffffffff
                check.slow_codes = int((dec_h >> 32).sum())     # LZW: strings copied through memory (sources older than the LDS ring)
                bad = np.nonzero((st_h != 0) | (produced != expect))[0]
                if bad.size:
                    b = int(bad[0])
                    per = nb // len(planes)
                    # the block's number in the file (planes that were left out count, and the blocks around a window's sub-grid)
                    fb = planes[b // per] * self._nx * self._ny + (by0 + b % per // nx) * self._nx + bx0 + b % per % nx
                    if self.compression in (8, 32946) and int(st_h[b]) == 3:
                        raise ValueError(f"{self.path}: block {fb}: Adler-32 mismatch (status 3): its {int(produced[b])} decoded bytes do not sum to the stream's trailer")
                    if self.compression == 50000 and int(st_h[b]) == 4:
                        raise ValueError(f"{self.path}: block {fb}: declined by the device decoder (status 4): a content checksum, a second frame or a skippable frame")
                    raise ValueError(f"{self.path}: block {fb} decodes to {int(produced[b])} bytes (status {int(st_h[b])}), expected {int(expect[b])}")
            keep = [pin, comp, meta, bufs]                 # alive until check() has run: the kernels read them
            return image, finish(image, k0, k1, [bufs.decoded, bufs.status[:nb]], keep, verdict, span, **where)

    def _jpeg_to_device(self, dev, pin, comp, lo, span, k0, k1, long_segments=False, long_threshold=None, subseq_bytes=None, where=None):
        """decode_to_device for JPEG blocks (inside its device / stream context, the compressed bytes already on their way to ``comp``):
        the plan's arrays go to the device, td_tiff_jpeg_decode_dev decodes (entropy segments one per lane, IDCT, upsampling + colour)
        straight into the raster. Same (image, check) contract; ``check()`` names the first block whose data is corrupt.
        ``long_segments``: the plan's segments are split at ``long_threshold`` bytes and td_tiff_jpeg_decode_long_dev decodes both lists."""
        import torch
        from . import _lib
        lib = _lib.load()
        info, segs, sets, ncoef = self._jpeg_plan()
        nb = len(info)
        segs = segs.copy()
        segs[:, 0] -= lo                                        # file offsets → offsets in the copied span
        info_d = torch.from_numpy(info).to(dev, non_blocking=True)
        segs_d = torch.from_numpy(segs).to(dev, non_blocking=True)
        sets_d = torch.from_numpy(sets).to(dev, non_blocking=True)
        coef = torch.empty((max(ncoef, 64),), dtype=torch.int16, device=dev)
        planes = torch.empty((max(ncoef, 64),), dtype=torch.uint8, device=dev)
        status = torch.empty((nb,), dtype=torch.int32, device=dev)
        image = torch.empty((self.height, self.width, self.count), dtype=torch.uint8, device=dev)
        st = _lib.stream_ptr()
        nlong, stats = 0, None
        if long_segments:
            limit = self.JPEG_DEVICE_MAX_SEGMENT if long_threshold is None else int(long_threshold)
            is_long = segs[:, 1] > limit
            nlong = int(is_long.sum())
            # (one upload: the short segments first, the long ones behind them, each list in the plan's order)
            segs_d = torch.from_numpy(np.concatenate([segs[~is_long], segs[is_long]])).to(dev, non_blocking=True)
            stats = torch.empty((4,), dtype=torch.int64, device=dev)
        k0.record()
        if long_segments:
            nshort = len(segs) - nlong
            _lib.check(lib.td_tiff_jpeg_decode_long_dev(comp.data_ptr(), info_d.data_ptr(), nb, segs_d.data_ptr() if nshort else None, nshort,
                                                        segs_d[nshort:].data_ptr() if nlong else None, nlong,
                                                        int(subseq_bytes or self.JPEG_SYNC_SUBSEQ), sets_d.data_ptr(), coef.data_ptr(),
                                                        planes.data_ptr(), ncoef, status.data_ptr(), stats.data_ptr(), image.data_ptr(),
                                                        self.width, self.height, self.count, self._bw, self._bh, self._nx, st),
                       "td_tiff_jpeg_decode_long_dev")
        else:
            _lib.check(lib.td_tiff_jpeg_decode_dev(comp.data_ptr(), info_d.data_ptr(), nb, segs_d.data_ptr(), len(segs), sets_d.data_ptr(),
                                                   coef.data_ptr(), planes.data_ptr(), ncoef, status.data_ptr(), image.data_ptr(), self.width,
                                                   self.height, self.count, self._bw, self._bh, self._nx, st), "td_tiff_jpeg_decode_dev")
        k1.record()                                        # entropy decode + IDCT + upsampling / colour

        def verdict(check, st_h, stats_h=None):
            if stats_h is not None:                        # rounds, windows, most rounds of a window, windows of one round
                check.sync_stats = [int(v) for v in stats_h]
                check.sync_rounds = check.sync_stats[0] / max(1, check.sync_stats[1])
            bad = np.nonzero(st_h != 0)[0]
            if bad.size:
                b = int(bad[0])
                raise ValueError(f"{self.path}: JPEG block {b} is corrupt (status {int(st_h[b])})")
        keep = [pin, comp, info_d, segs_d, sets_d, coef, planes, status, stats]     # alive until check() has run: the kernels read them
        return image, finish(image, k0, k1, [status] if stats is None else [status, stats], keep, verdict, span,
                             segments=len(segs), long_segments=nlong, sync_rounds=0.0, **(where or {}))

    def device_uploadable(self) -> bool:
        """True when the raster's pixels lie in the file as ONE dense [rows, cols, bands] array of uint8 or native-order uint16
        samples (uncompressed contiguous strips, pixel-interleaved): it can be copied to the GPU in large sequential pieces and
        its tile windows cut there. Big-endian, planar, int16 and float32 files keep the host reader."""
        self._setup_blocks()
        if self._flat is None or self._pil is not None or not self._device_samples():
            return False
        if getattr(self, "_fd", None) is not None:
            return True
        # (the window reader keeps a descriptor for single-byte samples only: a 16-bit file is checked for its length here)
        return self.dtype.itemsize == 2 and os.path.getsize(self.path) >= int(self._flat.offset) + self._flat.nbytes

    def upload_to_device(self, device, stream=None, staging=None, pool=None, piece: int = 4 << 20):
        """The whole uncompressed raster in HBM: the file's pixel bytes are read in large sequential pieces (pread of ``piece``
        bytes, several side by side on ``pool``) into pinned staging buffers and copied to the device as they arrive — per tile
        one memcpy of its bytes out of the page cache, no system call per window row and no per-batch H2D of windows later.
        ``staging``: list of >= 2 pinned uint8 tensors to rotate through (created here when None). → (image tensor [rows,
        cols, bands] uint8 or torch.uint16, check) as :meth:`decode_to_device`."""
        import torch
        if not self.device_uploadable():
            raise ValueError(f"{self.path}: not one dense uint8 / uint16 array in the file")
        dev = torch.device(device)
        total = self.height * self.width * self.count * self.dtype.itemsize        # bytes
        if staging is None:
            staging = [torch.empty((4 * piece,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        cap = min(t.numel() for t in staging)
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        base = int(self._flat.offset)
        with torch.cuda.device(dev), ctx:
            image = torch.empty((self.height, self.width, self.count), dtype=torch.uint8 if self.dtype.itemsize == 1 else torch.uint16, device=dev)
            flat = image.view(-1).view(torch.uint8)
            events = [None] * len(staging)
            k = 0
            for o in range(0, total, cap):
                n = min(cap, total - o)
                buf = staging[k % len(staging)]
                if events[k % len(staging)] is not None:
                    events[k % len(staging)].synchronize()          # the copy that last used this staging buffer has finished
                parts = [(p, min(piece, n - p), base + o + p) for p in range(0, n, piece)]
                # every piece goes to the device as soon as it (and the pieces before it) has been read: copies of a few MB keep
                # the DMA queue short for the small result copies of the running forwards (64-MB copies delayed them by a millisecond)
                for p0, pn, _ in read_ranges(self.path, parts, buf.numpy(), pool, "pixel data"):
                    flat[o + p0:o + p0 + pn].copy_(buf[p0:p0 + pn], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                events[k % len(staging)] = ev
                k += 1
            return image, finish(image, None, None, [], [], None, total)

    def _load(self) -> np.ndarray:
        """Whole raster as [bands, rows, cols]."""
        if self._data is None:
            self._data = self._window_hwc(0, 0, self.height, self.width).transpose(2, 0, 1)
        return self._data

    # -- rasterio-like surface ------------------------------------------------------------------------
    @property
    def bounds(self) -> Tuple[float, float, float, float]:
        a, _, c, _, e, f = self.transform
        return (c, f + e * self.height, c + a * self.width, f)   # left, bottom, right, top

    def read(self) -> np.ndarray:
        return np.asarray(self._load())

    def window_of_bounds(self, bounds: Sequence[float]) -> Tuple[int, int, int, int]:
        """rasterio.features.geometry_window for a bbox: floor / ceil in pixel space, clipped to the raster.
        Returns (col_off, row_off, width, height); width/height may be 0 when the bbox misses the raster."""
        a, _, c, _, e, f = self.transform
        minx, miny, maxx, maxy = (float(v) for v in bounds[:4])
        cols = [(minx - c) / a, (maxx - c) / a]
        rows = [(maxy - f) / e, (miny - f) / e]
        c0, c1 = int(math.floor(min(cols))), int(math.ceil(max(cols)))
        r0, r1 = int(math.floor(min(rows))), int(math.ceil(max(rows)))
        c0c, r0c = max(c0, 0), max(r0, 0)
        c1c, r1c = min(c1, self.width), min(r1, self.height)
        return c0c, r0c, max(c1c - c0c, 0), max(r1c - r0c, 0)

    def window_transform(self, col_off: int, row_off: int) -> Tuple[float, ...]:
        a, b, c, d, e, f = self.transform
        return (a, b, c + a * col_off + b * row_off, d, e, f + d * col_off + e * row_off)

    def _mask_outside(self, hwc: np.ndarray, bounds, c0: int, r0: int) -> None:
        """rasterio.mask semantics: pixels whose centre lies outside the bbox are set to 0."""
        h, w = hwc.shape[:2]
        a, _, c, _, e, f = self.transform
        minx, miny, maxx, maxy = (float(v) for v in bounds[:4])
        xs = c + a * (np.arange(c0, c0 + w) + 0.5)
        ys = f + e * (np.arange(r0, r0 + h) + 0.5)
        okx = (xs >= minx) & (xs <= maxx)
        oky = (ys >= miny) & (ys <= maxy)
        if not okx.all():
            hwc[:, ~okx, :] = 0
        if not oky.all():
            hwc[~oky, :, :] = 0

    def outside_mask(self, bounds, c0: int, r0: int, w: int, h: int):
        """The columns / rows of window (c0, r0, w, h) that ``_mask_outside`` keeps, as two boolean arrays — or None when it
        keeps everything (the usual case: tile bounds lie on pixel edges)."""
        a, _, c, _, e, f = self.transform
        minx, miny, maxx, maxy = (float(v) for v in bounds[:4])
        xs = c + a * (np.arange(c0, c0 + w) + 0.5)
        ys = f + e * (np.arange(r0, r0 + h) + 0.5)
        okx = (xs >= minx) & (xs <= maxx)
        oky = (ys >= miny) & (ys <= maxy)
        return None if okx.all() and oky.all() else (okx, oky)

    def read_bounds_hwc(self, bounds: Sequence[float], out: Optional[np.ndarray] = None, out_off: int = 0) -> np.ndarray:
        """``rasterio.mask.mask(img, [bbox], crop=True)[0]`` as pixel-interleaved [rows, cols, bands] — the layout the
        device resize consumes. With ``out`` (a flat array of the raster's dtype, e.g. pinned staging memory) the window
        is written at ``out_off`` and the returned array is a view of it. Raises ValueError when the bbox does not
        overlap the raster."""
        c0, r0, w, h = self.window_of_bounds(bounds)
        if w <= 0 or h <= 0:
            raise ValueError("Input shapes do not overlap raster.")
        dst = None if out is None else out[out_off:out_off + h * w * self.count].reshape(h, w, self.count)
        hwc = self._window_hwc(r0, c0, h, w, dst)
        self._mask_outside(hwc, bounds, c0, r0)
        return hwc

    def read_windows_flat(self, windows, out: np.ndarray, out_offs, threads: int = 8) -> bool:
        """The windows (col_off, row_off, width, height) of a whole batch of an uncompressed, pixel-interleaved raster in ONE library
        call (td_read_windows: pread per window row, row bands spread over ``threads`` C threads) into the flat array ``out`` at
        ``out_offs`` (elements). → False when the raster is not of that kind (the caller reads window by window)."""
        self._setup_blocks()
        if self._flat is None or getattr(self, "_fd", None) is None or out.dtype != self.dtype or not out.flags.c_contiguous:
            return False
        from . import _lib
        px = self.count * self.dtype.itemsize
        n = len(windows)
        foff = np.array([self._flat_off + (r0 * self.width + c0) * px for c0, r0, w, h in windows], dtype=np.int64)
        rbytes = np.array([w * px for c0, r0, w, h in windows], dtype=np.int64)
        rows = np.array([h for c0, r0, w, h in windows], dtype=np.int64)
        doff = np.asarray(out_offs, dtype=np.int64) * self.dtype.itemsize
        got = _lib.load().td_read_windows(self._fd, n, foff.ctypes.data, self.width * px, rbytes.ctypes.data, rows.ctypes.data, out.ctypes.data,
                                          doff.ctypes.data, int(threads))
        _lib.check(got, "td_read_windows")
        return True

    def read_bounds(self, bounds: Sequence[float]) -> np.ndarray:
        """Same window as [bands, rows, cols] (rasterio's axis order)."""
        return np.ascontiguousarray(self.read_bounds_hwc(bounds).transpose(2, 0, 1))


def device_decode_setting(value="auto"):
    """The ``device_decode`` config key as both stages read it (the Predictor's tile loop, the post-processing stage's height raster):
    true / false / "auto" / "all" → (use the device decoders, upload uncompressed rasters too). TD_DEVICE_DECODE (diagnostics: 0 |
    false | all) overrides the default "auto"; anything else is refused."""
    if value == "auto" and os.environ.get("TD_DEVICE_DECODE"):
        value = {"0": False, "false": False, "all": "all"}.get(os.environ["TD_DEVICE_DECODE"], "auto")
    if value not in (True, False, "auto", "true", "false", "all"):
        raise ValueError(f"device_decode must be true, false, 'auto' or 'all', got {value!r}")
    return value in (True, "auto", "true", "all"), value == "all"


def _true_false_setting(key, value) -> bool:
    if value is None:
        value = False
    if not any(value is v for v in (True, False)) and value not in ("true", "false"):
        raise ValueError(f"{key} must be true or false, got {value!r}")
    return value in (True, "true")


def device_decode_long_jpeg_setting(value=False) -> bool:
    """The ``device_decode_long_jpeg`` config key as both stages read it: true / false (default) → whether JPEG rasters with segments
    beyond GeoTiff.JPEG_DEVICE_MAX_SEGMENT go to the device too (``device_decodable(long_segments=True)``), where ``device_decode``
    sends rasters there at all. Anything else is refused."""
    return _true_false_setting("device_decode_long_jpeg", value)


def device_decode_planar_setting(value=False) -> bool:
    """The ``device_decode_planar`` config key as both stages read it: true / false (default) → whether band-separate rasters
    (PlanarConfiguration = 2) go to the device decoders too (``device_decodable(planar=True)``), where ``device_decode`` sends rasters
    there at all. Anything else is refused."""
    return _true_false_setting("device_decode_planar", value)


def _jpeg_block(blk: np.ndarray, quality: int = 90, subsampling: int = 2, restart: int = 0) -> bytes:
    """One strip / tile as a COMPLETE JPEG stream (its own tables: the JPEGTables tag is optional, TIFF Technical Note 2), YCbCr 4:2:0
    for three bands (``subsampling`` 0 = 4:4:4, 1 = 4:2:2), four bands as four components sampled 1x1 and stored as they are (Pillow's
    CMYK encoder inverts what it is given, Adobe's polarity, so it is given the inverse), a restart marker every ``restart`` MCUs
    when > 0 — Pillow's libjpeg encoder. Lossy: a test fixture for the windowed JPEG reader, not an archive format."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": int(restart)} if restart else {}
    if blk.shape[2] == 4:
        im = Image.frombytes("CMYK", (blk.shape[1], blk.shape[0]), (255 - blk).tobytes())
    else:
        im = Image.fromarray(blk[:, :, 0] if blk.shape[2] == 1 else blk)
    im.save(buf, "JPEG", quality=quality, subsampling=subsampling if blk.shape[2] == 3 else 0, **kw)
    return buf.getvalue()


def _jpeg_split(stream: bytes) -> Tuple[bytes, bytes]:
    """A complete JPEG stream → (its tables as a JPEGTables tag: SOI, DQT / DHT segments, EOI; the abbreviated stream without them
    and without JFIF or Adobe segment) — the layout GDAL / libtiff write (TIFF Technical Note 2)."""
    tables, rest = [b"\xff\xd8"], [b"\xff\xd8"]
    pos = 2
    while pos < len(stream):
        m = stream[pos + 1]
        if m == 0xDA:                                       # SOS: the scan and everything after it stay in the block
            rest.append(stream[pos:])
            break
        n = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        seg = stream[pos:pos + 2 + n]
        if m in (0xDB, 0xC4):
            tables.append(seg)
        elif m not in (0xE0, 0xEE):
            rest.append(seg)
        pos += 2 + n
    return b"".join(tables) + b"\xff\xd9", b"".join(rest)


_zstd_compress = None


def _libzstd_compressor():
    """→ compress(raw, level) by libzstd's ZSTD_compress, loaded on first use through ctypes: the system's library, else the copy
    bundled with Pillow. The writer's only; ValueError when neither loads."""
    global _zstd_compress
    if _zstd_compress is not None:
        return _zstd_compress
    import ctypes
    import ctypes.util
    import glob
    names = [ctypes.util.find_library("zstd")]
    try:
        import PIL
        names += sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libzstd*.so*")))
    except ImportError:
        pass
    z = None
    for name in names:
        try:
            # (RTLD_DEEPBIND: its internal calls stay inside it whatever other libzstd build the process has in its global scope)
            z = ctypes.CDLL(name, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND) if name else None
            if z is not None and all(hasattr(z, f) for f in ("ZSTD_compress", "ZSTD_compressBound", "ZSTD_isError")):
                break
            z = None
        except OSError:
            z = None
    if z is None:
        raise ValueError("compression='zstd': libzstd was not found (neither a system library nor Pillow's bundled copy loads)")
    z.ZSTD_compressBound.restype, z.ZSTD_compressBound.argtypes = ctypes.c_size_t, [ctypes.c_size_t]
    z.ZSTD_isError.restype, z.ZSTD_isError.argtypes = ctypes.c_uint, [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def compress(raw: bytes, level: int) -> bytes:
        out = ctypes.create_string_buffer(z.ZSTD_compressBound(len(raw)))
        n = z.ZSTD_compress(out, len(out), raw, len(raw), level)
        if z.ZSTD_isError(n):
            raise ValueError(f"ZSTD_compress failed at level {level}")
        return out.raw[:n]
    _zstd_compress = compress
    return compress


def write_geotiff(path: str, data: np.ndarray, transform: Sequence[float], epsg: int = 25832, *,
                  tile: Optional[Tuple[int, int]] = None, rows_per_strip: Optional[int] = None,
                  compression: Optional[str] = None, predictor: int = 1, planar: bool = False,
                  nodata: Optional[float] = None, jpeg_tables: bool = False, jpeg_restart: int = 0,
                  jpeg_quality: int = 90, jpeg_subsampling: int = 2, zstd_level: int = 9) -> None:
    """Classic little-endian TIFF with the GeoTIFF tags the reader understands. data: [bands, rows, cols] or
    [rows, cols]; uint8 / uint16 / uint32 (label rasters: SampleFormat 1, 32 bits; no JPEG, no predictor 3) / float32. Defaults: one uncompressed pixel-interleaved strip (what the tile reader
    maps without copying). Options: ``tile=(tile_rows, tile_cols)`` (multiples of 16) or ``rows_per_strip``,
    ``compression`` None / "deflate" / "lzw" (td_tiff_lzw_encode, blocks encoded on host threads) / "jpeg" (lossy; Pillow's encoder per
    block) / "zstd" (test rasters and the bench only: libzstd's one-shot ZSTD_compress at ``zstd_level`` through ctypes, the system's
    library or the copy bundled with Pillow; ValueError when neither loads — the reader never touches libzstd), ``predictor`` 1 / 2 (horizontal differencing; float32 samples are differenced as uint32, modulo 2^32, which is what libtiff's
    32-bit accumulator undoes) / 3 (floating-point predictor, TIFF Technical Note 3: float32 only), ``planar`` (one block grid per band). JPEG: ``jpeg_tables`` writes the GDAL / libtiff
    layout (the quantisation and Huffman tables once, in the JPEGTables tag; abbreviated blocks without JFIF) instead of complete
    streams; ``jpeg_restart`` > 0 puts a restart marker every that many MCUs; ``jpeg_quality``, ``jpeg_subsampling`` (2 = 4:2:0,
    1 = 4:2:2, 0 = 4:4:4 for three bands). Four bands: RGB + one unspecified extra sample (what GDAL writes for RGBI), four components
    sampled 1x1 without a colour transform."""
    arr = np.asarray(data)
    if arr.ndim == 2:
        arr = arr[None]
    C, H, W = arr.shape
    fmt = {np.dtype(np.uint8): (1, 8), np.dtype(np.uint16): (1, 16), np.dtype(np.uint32): (1, 32),
           np.dtype(np.float32): (3, 32)}[arr.dtype]
    if compression not in (None, "deflate", "lzw", "jpeg", "zstd"):
        raise ValueError("compression must be None, 'deflate', 'lzw', 'jpeg' or 'zstd'")
    if predictor not in (1, 2, 3):
        raise ValueError("predictor must be 1, 2 or 3")
    if predictor == 3 and fmt != (3, 32):
        raise ValueError("predictor 3 (floating-point predictor) needs float32 samples")
    hwc = np.ascontiguousarray(arr.transpose(1, 2, 0)).astype(arr.dtype.newbyteorder("<"), copy=False)
    if tile:
        bh, bw = int(tile[0]), int(tile[1])
        if bh % 16 or bw % 16:
            raise ValueError("tile sides must be multiples of 16")
    else:
        bh, bw = int(rows_per_strip or H), W
    if compression == "jpeg" and (planar or predictor != 1 or arr.dtype != np.uint8 or C not in (1, 3, 4) or bh % 16):
        raise ValueError("jpeg: uint8 grey / three-band / four-band chunky rasters, no predictor, block heights in multiples of 16")
    ny, nx = (H + bh - 1) // bh, (W + bw - 1) // bw
    blocks = []
    for p in range(C if planar else 1):
        src = hwc[:, :, p:p + 1] if planar else hwc
        for by in range(ny):
            for bx in range(nx):
                rows = bh if tile else min(bh, H - by * bh)
                blk = np.zeros((rows, bw, src.shape[2]), dtype=hwc.dtype)
                piece = src[by * bh:by * bh + rows, bx * bw:(bx + 1) * bw]
                blk[:piece.shape[0], :piece.shape[1]] = piece
                if predictor == 2:
                    ints = blk.view("<u4") if fmt[0] == 3 else blk          # float32: the bit patterns, modulo 2^32
                    ints[:, 1:] = ints[:, 1:] - ints[:, :-1]       # modulo the sample width
                elif predictor == 3:
                    # the samples' bytes in four planes per row, most significant first, then byte differences with the pixel stride
                    # over the whole row of planes (libtiff's fpDiff)
                    u = blk.view("<u4").reshape(rows, -1)
                    row = np.concatenate([(u >> s & 255).astype(np.uint8) for s in (24, 16, 8, 0)], axis=1)
                    row[:, src.shape[2]:] = row[:, src.shape[2]:] - row[:, :-src.shape[2]]
                    blk = row
                if compression == "jpeg":
                    blocks.append(_jpeg_block(blk, jpeg_quality, jpeg_subsampling, jpeg_restart))
                    continue
                raw = blk.tobytes()
                blocks.append(zlib.compress(raw, 6) if compression == "deflate" else raw)
    tables_tag = None
    if compression == "jpeg" and jpeg_tables:
        split = [_jpeg_split(b) for b in blocks]
        tables_tag = split[0][0]
        if any(t != tables_tag for t, _ in split):
            raise ValueError("jpeg_tables: the blocks do not share their tables")
        blocks = [b for _, b in split]
    if compression == "lzw":
        from . import _lib
        lib = _lib.load()

        def enc(raw: bytes) -> bytes:
            src = np.frombuffer(raw, dtype=np.uint8)
            dst = np.empty(len(raw) * 3 // 2 + 64, dtype=np.uint8)          # 12-bit codes for single bytes at worst
            n = lib.td_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, dst.size)
            _lib.check(n, "td_tiff_lzw_encode")
            return dst[:n].tobytes()
        with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
            blocks = list(ex.map(enc, blocks))
    if compression == "zstd":
        compress = _libzstd_compressor()
        blocks = [compress(raw, int(zstd_level)) for raw in blocks]
    a, _, c, _, e, f = (float(v) for v in transform[:6])
    entries = []   # (tag, type, count, payload bytes)

    def add(tag, typ, values):
        if typ == 2:                           # ASCII, NUL-terminated
            raw = values.encode("latin1") + b"\0"
            entries.append((tag, typ, len(raw), raw))
            return
        code = {3: "H", 4: "I", 7: "B", 12: "d"}[typ]
        entries.append((tag, typ, len(values), struct.pack("<" + str(len(values)) + code, *values)))

    add(256, 4, [W])
    add(257, 4, [H])
    add(258, 3, [fmt[1]] * C)
    add(259, 3, [{"deflate": 8, "lzw": 5, "jpeg": 7, "zstd": 50000}.get(compression, 1)])
    add(262, 3, [(6 if compression == "jpeg" and C == 3 else 2) if C >= 3 else 1])
    add(277, 3, [C])
    add(284, 3, [2 if planar else 1])
    if predictor != 1:
        add(317, 3, [predictor])
    if tile:
        add(322, 4, [bw])
        add(323, 4, [bh])
        add(324, 4, [0] * len(blocks))   # offsets, patched below
        add(325, 4, [len(b) for b in blocks])
    else:
        add(273, 4, [0] * len(blocks))   # offsets, patched below
        add(278, 4, [bh])
        add(279, 4, [len(b) for b in blocks])
    if C > 3:
        add(338, 3, [0] * (C - 3))
    add(339, 3, [fmt[0]] * C)
    if compression == "jpeg" and C == 3:
        add(530, 3, {0: [1, 1], 1: [2, 1]}.get(jpeg_subsampling, [2, 2]))       # YCbCrSubSampling: what _jpeg_block encodes
    if tables_tag is not None:
        add(347, 7, list(tables_tag))          # JPEGTables (UNDEFINED)
    add(33550, 12, [a, -e, 0.0])
    add(33922, 12, [0.0, 0.0, 0.0, c, f, 0.0])
    add(34735, 3, [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, int(epsg)])
    if nodata is not None:
        add(42113, 2, str(int(nodata)) if fmt == (1, 32) and float(nodata).is_integer() else repr(float(nodata)))
    entries.sort(key=lambda t: t[0])
    n = len(entries)
    ifd_off = 8
    extra_off = ifd_off + 2 + n * 12 + 4
    extra_len = sum(len(pl) + (len(pl) % 2) for _, _, _, pl in entries if len(pl) > 4)
    data_off = extra_off + extra_len
    offsets, pos = [], data_off
    for b in blocks:
        offsets.append(pos)
        pos += len(b) + (len(b) % 2)
    if pos >= 1 << 32:
        raise ValueError("raster too large for a classic TIFF")
    off_tag = 324 if tile else 273
    out = bytearray(struct.pack("<2sHI", b"II", 42, ifd_off))
    out += struct.pack("<H", n)
    extra = b""
    for tag, typ, cnt, payload in entries:
        if tag == off_tag:
            payload = struct.pack("<" + str(cnt) + "I", *offsets)
        if len(payload) <= 4:
            val = payload.ljust(4, b"\0")
        else:
            val = struct.pack("<I", extra_off + len(extra))
            extra += payload + (b"\0" if len(payload) % 2 else b"")
        out += struct.pack("<HHI", tag, typ, cnt) + val
    out += struct.pack("<I", 0)
    out += extra
    with open(path, "wb") as fh:
        fh.write(bytes(out))
        for b in blocks:
            fh.write(b)
            if len(b) % 2:
                fh.write(b"\0")
