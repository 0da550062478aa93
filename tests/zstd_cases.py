"""Shared pieces of the Zstandard tests (tests/test_zstd_decode.py, tests/test_zstd_decode_gpu.py, tests/golden/make_zstd_fixture.py):
the inputs the committed streams were made from, hand-built frames for the modes libzstd does not emit, seeded mutations, libzstd
through ctypes (the judge; CPU tests only), and thin wrappers of td_tiff_zstd_decode / td_zstd_stream_stats."""
import ctypes as C
import ctypes.util
import glob
import hashlib
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd")
MAGIC = b"\x28\xb5\x2f\xfd"

# every mode the committed streams must reach (counters of td_zstd_stream_stats); "blocks3" = a frame of three or more blocks
REQUIRED_MODES = ("block_raw block_rle block_comp blocks3 lit_raw lit_huff lit_treeless lit_streams_4 lit_streams_1 hufw_direct hufw_fse seq0 "
                  "LL_predef LL_rle LL_fse LL_repeat ML_predef ML_rle ML_fse ML_repeat OF_predef OF_rle OF_fse window_desc single_segment "
                  "checksum").split()


# ---- our decoder ---------------------------------------------------------------------------------------------------------------------
def decode(stream: bytes, cap: int):
    """td_tiff_zstd_decode → (status or byte count, bytes decoded)."""
    from treedetection_amd import _lib
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    n = lib.td_tiff_zstd_decode(src.ctypes.data, len(stream), dst.ctypes.data, cap)
    return int(n), (dst[:n].tobytes() if n >= 0 else b"")


def stats(stream: bytes):
    """td_zstd_stream_stats → (byte count or status, {name: count}) with "blocks3" added."""
    from treedetection_amd import _lib
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8).copy()
    cnt = np.zeros(len(_lib.ZSTD_STATS), dtype=np.int64)
    n = lib.td_zstd_stream_stats(src.ctypes.data, len(stream), cnt.ctypes.data)
    d = dict(zip(_lib.ZSTD_STATS, (int(v) for v in cnt)))
    d["blocks3"] = int(d["max_blocks_per_frame"] >= 3)
    return int(n), d


# ---- libzstd, the judge --------------------------------------------------------------------------------------------------------------
class _InBuf(C.Structure):
    _fields_ = [("src", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


class _OutBuf(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


class LibZstd:
    def __init__(self, path):
        # RTLD_DEEPBIND: the library's internal calls stay inside it even when another libzstd build is in the process's global scope
        # (libtreedet_hip.so is loaded RTLD_GLOBAL and the ROCm libraries bring the system's build with them)
        z = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        self.z = z
        for name, res, args in (("ZSTD_compressBound", C.c_size_t, [C.c_size_t]), ("ZSTD_isError", C.c_uint, [C.c_size_t]),
                                ("ZSTD_compress", C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]),
                                ("ZSTD_decompress", C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
                                ("ZSTD_versionNumber", C.c_uint, []), ("ZSTD_createCCtx", C.c_void_p, []), ("ZSTD_freeCCtx", C.c_size_t, [C.c_void_p]),
                                ("ZSTD_CCtx_setParameter", C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
                                ("ZSTD_compress2", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
                                ("ZSTD_compressStream2", C.c_size_t, [C.c_void_p, C.POINTER(_OutBuf), C.POINTER(_InBuf), C.c_int])):
            fn = getattr(z, name)
            fn.restype, fn.argtypes = res, args
        v = z.ZSTD_versionNumber()
        self.version = f"{v // 10000}.{v // 100 % 100}.{v % 100}"

    def compress(self, data: bytes, level: int) -> bytes:
        out = C.create_string_buffer(self.z.ZSTD_compressBound(len(data)))
        n = self.z.ZSTD_compress(out, len(out), data, len(data), level)
        assert not self.z.ZSTD_isError(n)
        return out.raw[:n]

    def compress_advanced(self, data: bytes, level: int, checksum: bool = False) -> bytes:
        cctx = self.z.ZSTD_createCCtx()
        try:
            assert not self.z.ZSTD_isError(self.z.ZSTD_CCtx_setParameter(cctx, 100, level))              # ZSTD_c_compressionLevel
            assert not self.z.ZSTD_isError(self.z.ZSTD_CCtx_setParameter(cctx, 201, int(checksum)))      # ZSTD_c_checksumFlag
            out = C.create_string_buffer(self.z.ZSTD_compressBound(len(data)))
            n = self.z.ZSTD_compress2(cctx, out, len(out), data, len(data))
            assert not self.z.ZSTD_isError(n)
            return out.raw[:n]
        finally:
            self.z.ZSTD_freeCCtx(cctx)

    def compress_stream(self, data: bytes, level: int, chunk: int = 50000) -> bytes:
        """The streaming API without a pledged size: a frame with a window descriptor and no content size."""
        cctx = self.z.ZSTD_createCCtx()
        try:
            assert not self.z.ZSTD_isError(self.z.ZSTD_CCtx_setParameter(cctx, 100, level))
            out = C.create_string_buffer(self.z.ZSTD_compressBound(len(data)) + 1024)
            ob = _OutBuf(C.cast(out, C.c_void_p), len(out), 0)
            src = C.create_string_buffer(data, len(data)) if data else C.create_string_buffer(1)
            pos = 0
            while True:
                end = min(len(data), pos + chunk)
                ib = _InBuf(C.cast(src, C.c_void_p).value + pos if pos else C.cast(src, C.c_void_p), end - pos, 0)
                last = end == len(data)
                while True:
                    rem = self.z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), 2 if last else 0)      # ZSTD_e_end / ZSTD_e_continue
                    assert not self.z.ZSTD_isError(rem)
                    if (last and rem == 0) or (not last and ib.pos == ib.size):
                        break
                pos = end
                if last:
                    return out.raw[:ob.pos]
        finally:
            self.z.ZSTD_freeCCtx(cctx)

    def decompress(self, stream: bytes, cap: int):
        """→ bytes, or None where libzstd refuses"""
        out = C.create_string_buffer(max(cap, 1))
        n = self.z.ZSTD_decompress(out, cap, stream, len(stream))
        return None if self.z.ZSTD_isError(n) else out.raw[:n]


def libzstd_paths():
    """The libzstd builds this machine has: the system's and the one bundled with Pillow."""
    paths = []
    sysname = ctypes.util.find_library("zstd")
    if sysname:
        paths.append(sysname)
    try:
        import PIL
        paths += sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libzstd*.so*")))
    except ImportError:
        pass
    return paths


_BUILDS = None


def libzstd_builds():
    global _BUILDS
    if _BUILDS is None:
        _BUILDS, seen = [], set()
        for p in libzstd_paths():
            try:
                z = LibZstd(p)
            except (OSError, AttributeError):
                continue
            if z.version not in seen:
                seen.add(z.version)
                _BUILDS.append(z)
    return _BUILDS


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def smooth_image(seed=11, side=256, bands=4, noise=2.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    img = np.zeros((side, side, bands))
    for c in range(bands):
        for _ in range(4):
            img[:, :, c] += 28 * np.cos(rng.uniform(0.01, 0.09) * xx + rng.uniform(0.01, 0.09) * yy + rng.uniform(0, 6))
    img += rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img + 120), 0, 255).astype(np.uint8)


def hdiff(img):
    out = img.copy()
    out[:, 1:] = img[:, 1:] - img[:, :-1]
    return out


def label_signal(seed=5, n=300000):
    rng = np.random.default_rng(seed)
    out = np.empty(n + 200, dtype=np.uint8)
    pos = 0
    while pos < n:
        run = int(rng.integers(1, 200))
        out[pos:pos + run] = rng.integers(0, 6)
        pos += run
    return out[:n].tobytes()


def periodic(period: int, n: int, seed=3) -> bytes:
    base = np.random.default_rng(seed + period).integers(0, 256, period, dtype=np.uint8)
    return np.resize(base, n).tobytes()


PERIODS = (1, 2, 3, 5, 7, 63, 64, 65, 100)


def inputs():
    """name → bytes: the inputs of the committed streams (tests/golden/make_zstd_fixture.py)."""
    rng = np.random.default_rng(2024)
    img = smooth_image()
    d = {"zeros": bytes(300000), "noise": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(), "image": img.tobytes(),
         "image_diff": hdiff(img).tobytes(), "image64": np.ascontiguousarray(img[:64, :64]).tobytes(),
         "image64_diff": hdiff(np.ascontiguousarray(img[:64, :64])).tobytes(), "image16": np.ascontiguousarray(img[:16, :16]).tobytes(),
         "image16_diff": hdiff(np.ascontiguousarray(img[:16, :16])).tobytes()}
    t = np.arange(131072)
    sine = np.rint(20000 + 9000 * np.sin(t / 37.0) + rng.normal(0, 6, t.size)).astype(np.uint16)
    d["sine16_diff"] = np.diff(sine, prepend=sine[:1]).astype(np.uint16).tobytes()
    d["arange3"] = (np.arange(75000, dtype=np.uint32) * 3).tobytes()
    row = rng.integers(0, 256, 1024, dtype=np.uint8)
    rows = np.tile(row, (256, 1))
    flip = rng.random(rows.shape) < 0.02
    rows[flip] ^= (1 << rng.integers(0, 8, int(flip.sum()))).astype(np.uint8)
    d["rows_flipped"] = rows.tobytes()
    rec = np.empty((37000, 7), dtype=np.uint8)
    rec[:, :4] = rng.integers(0, 256, (37000, 1), dtype=np.uint8)
    rec[:, 4:] = rng.integers(0, 256, (37000, 3), dtype=np.uint8)
    d["records"] = rec.tobytes()
    d["labels"] = label_signal()
    for p in PERIODS:
        d[f"period{p}_700"] = periodic(p, 700)
    d["period7_210000"] = periodic(7, 210000)
    return d


# ---- hand-built frames ----------------------------------------------------------------------------------------------------------------
def block(kind: int, body: bytes, size=None, last=True) -> bytes:
    """Block header (3 bytes) + body; kind 0 raw, 1 RLE, 2 compressed, 3 reserved. size: Block_Size (default: len(body))."""
    size = len(body) if size is None else size
    return struct.pack("<I", int(last) | kind << 1 | size << 3)[:3] + body


def frame(blocks: bytes, *, single=False, fcs=None, fcs_bytes=0, window_log=17, window_mant=0, checksum=None, did=b"", reserved=False,
          unused=False) -> bytes:
    """A frame header in any of its forms + the blocks (+ a checksum of four bytes)."""
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert fcs_bytes != 1 or single
    fhd = flag << 6 | int(single) << 5 | int(unused) << 4 | int(reserved) << 3 | int(checksum is not None) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[len(did)]
    out = MAGIC + bytes([fhd])
    if not single:
        out += bytes([(window_log - 10) << 3 | window_mant])
    out += did
    if fcs_bytes:
        out += int(fcs - 256 if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    out += blocks
    if checksum is not None:
        out += struct.pack("<I", checksum)
    return out


def rle_literals_block(byte: int, count: int, last=True) -> bytes:
    """A Compressed block of RLE literals and no sequences: `count` (< 4096) times `byte`."""
    head = struct.pack("<H", 1 | 1 << 2 | count << 4) if count > 31 else bytes([1 | count << 3])
    return block(2, head + bytes([byte, 0]), last=last)


def raw_literals(data: bytes) -> bytes:
    n = len(data)
    if n < 32:
        return bytes([n << 3]) + data
    if n < 4096:
        return struct.pack("<H", 1 << 2 | n << 4) + data
    return struct.pack("<I", 3 << 2 | n << 4)[:3] + data


class _BackWriter:
    """A backward bit stream: fields are written in the order the decoder reads them LAST to FIRST."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= value << self.n
        self.n += bits

    def done(self) -> bytes:
        self.put(1, 1)
        return self.v.to_bytes((self.n + 7) // 8, "little")


def sequences_rle_block(literals: bytes, seqs, of_mode_repeat=False, last=True) -> bytes:
    """A Compressed block of raw literals whose sequences all share ONE (ll code, of code, ml code): RLE mode for the three tables (or
    repeat mode for the offsets: of_mode_repeat) — seqs: list of (ll_extra, of_extra, ml_extra) with codes (llc, ofc, mlc) in seqs.codes."""
    llc, ofc, mlc = seqs.codes
    ll_bits = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    ml_bits = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    n = len(seqs)
    head = bytes([n]) if n < 128 else (bytes([128 + (n >> 8), n & 255]) if n < 0x7F00 else b"\xff" + struct.pack("<H", n - 0x7F00))
    modes = 1 << 6 | (3 if of_mode_repeat else 1) << 4 | 1 << 2
    tables = bytes([llc]) + (b"" if of_mode_repeat else bytes([ofc])) + bytes([mlc])
    w = _BackWriter()
    for ll_x, of_x, ml_x in reversed(seqs):                       # the decoder reads: offset bits, match bits, literal bits (states take 0 bits)
        w.put(ll_x, ll_bits[llc])
        w.put(ml_x, ml_bits[mlc])
        w.put(of_x, ofc)
    return block(2, raw_literals(literals) + head + bytes([modes]) + tables + w.done(), last=last)


class Seqs(list):
    def __init__(self, codes, items):
        super().__init__(items)
        self.codes = codes


def hand_frames():
    """name → (frame bytes, expected output or None where it must be refused, "host only" flag: the device declines it)."""
    out = {}
    pay = bytes(range(200)) + b"tail"
    raw = block(0, pay)
    out["hdr_single_fcs1"] = (frame(raw, single=True, fcs=len(pay), fcs_bytes=1), pay, False)
    for fb in (2, 4, 8):
        big = pay * 2                                              # 408 bytes: the 2-byte form stores size - 256
        out[f"hdr_single_fcs{fb}"] = (frame(block(0, big), single=True, fcs=len(big), fcs_bytes=fb), big, False)
        out[f"hdr_window_fcs{fb}"] = (frame(block(0, big), fcs=len(big), fcs_bytes=fb), big, False)
    out["hdr_window_nofcs"] = (frame(raw, window_log=10, window_mant=3), pay, False)
    out["hdr_unused_bit"] = (frame(raw, unused=True), pay, False)
    out["hdr_fcs_wrong"] = (frame(raw, single=True, fcs=len(pay) + 1, fcs_bytes=1), None, False)
    out["hdr_reserved_bit"] = (frame(raw, reserved=True), None, False)
    for did in (b"\x07", b"\x07\x00", b"\x07\x00\x00\x00"):
        out[f"hdr_dictionary{len(did)}"] = (frame(raw, did=did), None, False)
    out["hdr_did0"] = (frame(raw, did=b"\x00"), pay, False)
    out["block_reserved"] = (frame(block(3, pay)), None, False)
    out["block_beyond_window"] = (frame(block(0, bytes(1500)), window_log=10), None, False)
    out["three_blocks"] = (frame(block(0, b"abc", last=False) + block(1, b"z", size=1000, last=False) + block(0, b"end")), b"abc" + b"z" * 1000 + b"end", False)
    out["rle_literals"] = (frame(block(0, b"ab", last=False) + rle_literals_block(0x5A, 900)), b"ab" + b"\x5a" * 900, False)
    out["rle_literals_short"] = (frame(rle_literals_block(0x11, 7)), b"\x11" * 7, False)
    # sequences with all three tables in RLE mode: 5 literals + a match of 3 + 7 at offset (1 << 2) + 1 - 3 = 2 ... each
    lit = b"HELLO" * 3 + b"!"
    s = Seqs((5, 2, 7), [(0, 1, 0)] * 3)                           # ll 5, offset value 4 + 1 = 5 → offset 2, match 10
    exp = bytearray()
    for k in range(3):
        exp += lit[5 * k:5 * k + 5]
        for _ in range(10):
            exp.append(exp[-2])
    exp += b"!"
    out["seq_rle_modes"] = (frame(sequences_rle_block(lit, s)), bytes(exp), False)
    # offsets in repeat mode: the second block repeats the first one's RLE offset table
    out["seq_of_repeat"] = (frame(sequences_rle_block(lit, s, last=False) + sequences_rle_block(lit, s, of_mode_repeat=True)), bytes(exp) * 2, False)
    out["seq_of_repeat_first"] = (frame(sequences_rle_block(lit, s, of_mode_repeat=True)), None, False)
    # a sequence count above 0x7EFF (the three-byte form): 33 000 matches of 3 bytes at offset 1 behind a raw block of one byte
    s3 = Seqs((0, 2, 0), [(0, 0, 0)] * 33000)                      # ll 0, offset value 4 → offset 1, match 3
    out["seq_count_long"] = (frame(block(0, b"q", last=False) + sequences_rle_block(b"", s3)), b"q" + b"q" * 99000, False)
    out["seq_count_2byte"] = (frame(block(0, b"q", last=False) + sequences_rle_block(b"", Seqs((0, 2, 0), [(0, 0, 0)] * 300))), b"q" * 901, False)
    out["offset_too_far"] = (frame(sequences_rle_block(b"ab", Seqs((2, 3, 0), [(0, 0, 0)]))), None, False)
    # what only the host takes
    skip = struct.pack("<II", 0x184D2A53, 5) + b"\x01\x02\x03\x04\x05"
    one = frame(raw, single=True, fcs=len(pay), fcs_bytes=1)
    out["skippable_first"] = (skip + one, pay, True)
    out["skippable_last"] = (one + skip, pay, True)
    out["two_frames"] = (one + frame(block(1, b"k", size=50)), pay + b"k" * 50, True)
    out["skippable_truncated"] = (one + skip[:-1], None, True)
    out["trailing_garbage"] = (one + b"\x00\x01\x02\x03\x04", None, False)
    return out


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
def flip_bits(n: int, count: int):
    """The first `count` bit positions the sanitizer program (csrc/checks/zstd_check.cpp) flips in a stream of n bytes: one generator for
    both, so that every damaged stream a test feeds to the kernel is one the program has passed on the host. A 64-bit linear congruential
    sequence seeded by the stream's size."""
    seed, out = (0x9E3779B97F4A7C15 ^ n) & 0xFFFFFFFFFFFFFFFF, []
    for _ in range(count):
        seed = (seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out.append((seed >> 24) % (n * 8))
    return out


def mutations(stream: bytes, seed: int, prefixes: int, flips: int):
    """Seeded prefixes (the sanitizer program runs every prefix) and the first `flips` single-bit flips of flip_bits()."""
    rng = np.random.default_rng(seed)
    out = []
    for cut in sorted(set(int(v) for v in rng.integers(0, len(stream), prefixes))):
        out.append(stream[:cut])
    for pos in flip_bits(len(stream), flips):
        b = bytearray(stream)
        b[pos >> 3] ^= 1 << (pos & 7)
        out.append(bytes(b))
    return out


def committed_hand_frames():
    """name → (frame bytes as committed under tests/golden/zstd, expected output or None, host-only flag): hand_frames() read back
    from the files the sanitizer program runs over (tests/test_zstd_decode.py holds the two equal)."""
    built = hand_frames()
    out = {}
    for e in manifest()["hand"]:
        with open(os.path.join(GOLDEN, e["file"]), "rb") as f:
            out[e["name"]] = (f.read(), built[e["name"]][1], built[e["name"]][2])
    return out


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def load_stream(entry) -> bytes:
    with open(os.path.join(GOLDEN, entry["file"]), "rb") as f:
        return f.read()


def sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()
