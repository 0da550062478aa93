"""Float32 height rasters for the predictor tests (tests/test_f32_predictor.py, tests/test_f32_device_gpu.py): a synthetic nDSM
with a block of uniformly random BIT PATTERNS in it — NaNs with payloads, infinities, denormals and -0.0 occur — and the
floating-point predictor (TIFF Technical Note 3) restated in numpy, encoder and decoder, independent of the package's C and HIP."""
import struct

import numpy as np

from treedetection_amd.synth import make_tile

T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)
LAYOUTS = {"tile128": {"tile": (128, 128)}, "tile64x256": {"tile": (64, 256)}, "strip7": {"rows_per_strip": 7}, "strip1": {"rows_per_strip": 1}}


def bits(a) -> np.ndarray:
    """The samples as uint32: float ``==`` says NaN != NaN and -0.0 == 0.0."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def height_raster(bands: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """→ float32 [bands, h, w]: band b is the nDSM of synthetic tile seed + b; a block of random bit patterns lies across the
    first block boundaries of every layout, and NaN, +-Inf, -0.0 and the smallest denormal are planted in the corners."""
    rng = np.random.default_rng(100 + seed)
    size = max(h, w)
    out = np.stack([make_tile(seed + b, size)[1][:h, :w] for b in range(bands)]).astype(np.float32)
    r0, c0, rh, rw = min(50, h // 3), min(100, w // 3), min(90, h - h // 3), min(180, w - w // 3)
    noise = rng.integers(0, 1 << 32, (bands, rh, rw), dtype=np.uint64).astype(np.uint32)
    out[:, r0:r0 + rh, c0:c0 + rw] = noise.view(np.float32)
    special = np.array([0x7fc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0xffffffff], dtype=np.uint32).view(np.float32)
    for b in range(bands):
        out[b, 0, :min(6, w)] = special[:min(6, w)]
        out[b, -1, -min(6, w):] = special[:min(6, w)]
    got = bits(out)
    assert (np.isnan(out).any() and np.isinf(out).any() and (got == 0x80000000).any()
            and (((got & 0x7f800000) == 0) & ((got & 0x007fffff) != 0)).any())
    return out


def fp_encode(block: np.ndarray) -> np.ndarray:
    """float32 [rows, cols, samples] → the bytes of a predictor-3 block, uint8 [rows, 4 * cols * samples]: per row the samples'
    bytes sorted into four planes, most significant first, then every byte minus the byte ``samples`` before it (modulo 256)
    over the whole row of planes."""
    rows, cols, spp = block.shape
    be = bits(block).astype(">u4").view(np.uint8).reshape(rows, cols * spp, 4)       # big-endian bytes of the bit patterns
    planes = be.transpose(0, 2, 1).reshape(rows, 4 * cols * spp)
    out = planes.copy()
    out[:, spp:] = planes[:, spp:] - planes[:, :-spp]
    return out


def fp_decode(data: np.ndarray, rows: int, cols: int, spp: int) -> np.ndarray:
    """The inverse: uint8 [rows * 4 * cols * samples] → float32 [rows, cols, samples]."""
    n = cols * spp
    b = np.array(data, dtype=np.uint8).reshape(rows, 4 * n)
    for c in range(spp):                                    # the running sum of every channel's bytes, across the plane boundaries
        b[:, c::spp] = np.cumsum(b[:, c::spp], axis=1, dtype=np.uint8)
    be = b.reshape(rows, 4, n).transpose(0, 2, 1)
    return np.ascontiguousarray(be).view(">u4").astype(np.uint32).view(np.float32).reshape(rows, cols, spp)


def to_big_endian(src, dst):
    """A classic little-endian TIFF as write_geotiff lays it out (one IFD at 8) → the same file big-endian: every header field, tag entry
    and out-of-line tag value byte-swapped at its width; pixel data untouched (so: only right for data whose bytes do not depend on
    the byte order — predictor 3 — or for callers that swap the samples themselves)."""
    raw = bytearray(open(src, "rb").read())
    assert raw[:4] == b"II*\0"
    ifd = struct.unpack("<I", raw[4:8])[0]
    n = struct.unpack("<H", raw[ifd:ifd + 2])[0]
    out = bytearray(raw)
    out[:8] = b"MM" + struct.pack(">HI", 42, ifd)
    out[ifd:ifd + 2] = struct.pack(">H", n)
    size = {1: 1, 2: 1, 3: 2, 4: 4, 7: 1, 12: 8}
    for i in range(n):
        e = ifd + 2 + 12 * i
        tag, typ, cnt = struct.unpack("<HHI", raw[e:e + 8])
        out[e:e + 8] = struct.pack(">HHI", tag, typ, cnt)
        total = size[typ] * cnt
        if total <= 4:
            pos = e + 8
        else:
            pos = struct.unpack("<I", raw[e + 8:e + 12])[0]
            out[e + 8:e + 12] = struct.pack(">I", pos)
        w = size[typ]
        for k in range(cnt if w > 1 else 0):
            out[pos + k * w:pos + (k + 1) * w] = raw[pos + k * w:pos + (k + 1) * w][::-1]
    open(dst, "wb").write(bytes(out))


def patch_tag(path, tag, values):
    """Overwrite the values of one tag of a little-endian classic TIFF in place (same type and count as written)."""
    raw = bytearray(open(path, "rb").read())
    ifd = struct.unpack("<I", raw[4:8])[0]
    size = {3: ("H", 2), 4: ("I", 4)}
    for i in range(struct.unpack("<H", raw[ifd:ifd + 2])[0]):
        e = ifd + 2 + 12 * i
        t, typ, cnt = struct.unpack("<HHI", raw[e:e + 8])
        if t == tag:
            code, w = size[typ]
            assert cnt == len(values)
            pos = e + 8 if w * cnt <= 4 else struct.unpack("<I", raw[e + 8:e + 12])[0]
            raw[pos:pos + w * cnt] = struct.pack("<" + str(cnt) + code, *values)
            open(path, "wb").write(bytes(raw))
            return
    raise KeyError(tag)


def write_float64(path, data, transform, **kw):
    """A float64 [rows, cols] raster in strips: written as float32 pairs [rows, 2 cols] (the same bytes), then ImageWidth and
    BitsPerSample say what they are. (write_geotiff has no float64; the geo tags' pixel size is set for the true width.)"""
    from treedetection_amd.geotiff import write_geotiff
    d = np.ascontiguousarray(data, dtype=np.float64)
    assert "tile" not in kw and kw.get("predictor", 1) == 1
    write_geotiff(path, d.view(np.float32)[None], transform, 25832, **kw)
    patch_tag(path, 256, [d.shape[1]])
    patch_tag(path, 258, [64])
