"""Crafted block sets for the device JPEG decoder (jpegdecode.hip) and ONE checker, shared by tests/test_jpeg_cases.py (CPU: the cases
mean what they claim, the checker rejects what a wrong kernel would give) and tests/test_jpeg_cases_gpu.py (the kernels on them).

A case is a grid of COMPLETE JPEG streams, one per block, each with tables of its own: what write_geotiff never produces — several
table sets, sampling modes and coefficient counts in one launch, optimised Huffman tables, steps of 255, frames taller than their
block, rasters of a few pixels, counts at the wave boundary, and every 5th bit of the entropy-coded data flipped. The expected image is
Pillow's libjpeg on every block (the flips: the host twin td_jpeg_decode, status included), cropped to the raster and laid in the grid.
Nothing here imports torch at module level: the CPU tests use the cases, the plan and the checker without a device."""
import io
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
from PIL import Image, ImageFile

from treedetection_amd import _lib

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
MODE_OF = {"L": 0, "444": 1, "422": 2, "420": 3}
GUARD = 4096                                   # canary elements on either side of every device buffer
DEFAULT_SUBSEQ = 256                           # GeoTiff.JPEG_SYNC_SUBSEQ
POOL_SIZE = 10                                 # P: the restage family's streams, pairwise distinct table sets
TINY_SIZES = [(1, 1), (2, 3), (3, 5), (5, 4), (9, 2), (33, 1), (7, 13), (17, 33)]
TINY_MODES = ["L", "444", "422", "420"]
WAVE_DC = ["grey-63", "grey-64", "grey-65", "420-128x128"]
WAVE_TARGETS = [1, 2, 63, 64, 65, 128, 129]
FLIP_STREAMS = ["420-q90-smooth", "422-q75-restart2", "444-q60-optimize"]
FLIP_STRIDE = 5


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
def image(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    """The generators of tests/test_jpeg_decode.py: uniform noise, or a smooth field under a little noise. [h, w, 3] uint8."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def image4(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    return np.concatenate([image(h, w, kind, seed), image(h, w, kind, seed + 1000)[:, :, :1]], axis=2)


def encode(img: np.ndarray, mode: str, **kw) -> bytes:
    """Pillow's libjpeg encoder as tests/test_jpeg_decode.py::encode calls it; mode "4": four components sampled 1x1, stored as they
    are (geotiff._jpeg_block: Pillow's CMYK encoder inverts what it is given, so it is given the inverse)."""
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        buf = io.BytesIO()
        if mode == "L":
            Image.fromarray(img[:, :, 0]).save(buf, "JPEG", **kw)
        elif mode == "4":
            Image.frombytes("CMYK", (img.shape[1], img.shape[0]), (255 - img).tobytes()).save(buf, "JPEG", subsampling=0, **kw)
        else:
            Image.fromarray(img).save(buf, "JPEG", subsampling=SUBSAMPLING[mode], **kw)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def pillow(stream: bytes) -> np.ndarray:
    """Pillow's decode → [h, w, bands]; four components as geotiff._decode_jpeg_block reads them (raw mode CMYK: no inversion)."""
    with Image.open(io.BytesIO(stream)) as im:
        if im.mode == "CMYK":
            im.tile = [(t[0], t[1], t[2], ("CMYK",) + tuple(t[3][1:])) for t in im.tile]
        arr = np.asarray(im)
    return arr[:, :, None] if arr.ndim == 2 else arr


_OUT = np.zeros(1 << 18, dtype=np.uint8)


def _host(name: str, stream: bytes, *extra):
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8)
    shape = np.zeros(3, dtype=np.int32)
    n = getattr(lib, name)(src.ctypes.data, src.size, _OUT.ctypes.data, _OUT.size, shape.ctypes.data, *extra)
    if n < 0:
        return int(n)
    h, w, c = (int(v) for v in shape)
    assert n == h * w * c
    return _OUT[:n].reshape(h, w, c).copy()


def host_decode(stream: bytes):
    """td_jpeg_decode → [h, w, c] uint8, or the negative error code."""
    return _host("td_jpeg_decode", stream)


def host_decode_sync(stream: bytes, subseq: int, lanes: int = 64):
    """td_jpeg_decode_sync → ([h, w, c] or the error code, its four stats as a list)."""
    st = np.zeros(4, dtype=np.int64)
    got = _host("td_jpeg_decode_sync", stream, int(subseq), int(lanes), st.ctypes.data)
    return got, [int(v) for v in st]


def entropy_span(stream: bytes):
    """[start, end) of the entropy-coded data: from the end of the SOS header to before EOI."""
    sos = stream.index(b"\xff\xda")
    return sos + 2 + ((stream[sos + 2] << 8) | stream[sos + 3]), len(stream) - 2


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    blocks: List[bytes]                        # complete JPEG streams, row-major in the grid
    across: int                                # blocks_across
    bw: int
    bh: int
    width: int                                 # the raster: may crop the last column and row of blocks
    height: int
    bands: int
    refs: List[Optional[np.ndarray]] = field(repr=False, default_factory=list)   # per block: its decoded frame, None = not compared
    expected: np.ndarray = field(repr=False, default=None)

    def rect(self, b: int):
        """(y0, x0, rows, cols) of block b in the raster."""
        by, bx = divmod(b, self.across)
        y0, x0 = by * self.bh, bx * self.bw
        return y0, x0, min(self.bh, self.height - y0), min(self.bw, self.width - x0)

    def block_rows(self) -> np.ndarray:
        return np.array([self.rect(b)[2] for b in range(len(self.blocks))], dtype=np.int32)


def make_case(name, blocks, across, bw, bh, width, height, bands, refs=None) -> Case:
    assert len(blocks) % across == 0 and (across - 1) * bw < width <= across * bw
    down = len(blocks) // across
    assert (down - 1) * bh < height <= down * bh
    if refs is None:
        cache = {}
        refs = [cache.setdefault(s, pillow(s)) for s in blocks]
    case = Case(name, list(blocks), across, bw, bh, width, height, bands, list(refs))
    case.expected = np.zeros((height, width, bands), dtype=np.uint8)
    for b, ref in enumerate(refs):
        if ref is None:
            continue
        y0, x0, rows, cols = case.rect(b)
        assert ref.shape[0] >= rows and ref.shape[1] >= cols and ref.shape[2] == bands, (name, b, ref.shape)
        case.expected[y0:y0 + rows, x0:x0 + cols] = ref[:rows, :cols]
    return case


# 1. mixed: a 3 x 3 grid of 48 x 32 blocks in a 131 x 85 raster (right column cropped to 35, bottom row to 21). The grid has nine places
# and the last one repeats block 0's stream (two blocks, one table set), so the kinds share the other eight: every sampling mode,
# qualities 1 .. 100, optimised tables, steps of 255, restart intervals of 1 and 2 MCUs, and at place 4 (the middle: all 32 rows and 48 columns kept) one frame of 48 rows.
MIXED = {
    "rgb": [("444", "smooth", 32, dict(quality=90)),
            ("422", "noise", 32, dict(quality=75)),
            ("420", "smooth", 32, dict(quality=50, restart_marker_blocks=2)),
            ("420", "noise", 32, dict(quality=1)),
            ("422", "smooth", 48, dict(quality=85, restart_marker_blocks=1)),
            ("422", "noise", 32, dict(quality=95, optimize=True)),
            ("420", "smooth", 32, dict(qtables=[[255] * 64, [255] * 64])),
            ("444", "noise", 32, dict(quality=100))],
    "grey": [("L", "smooth", 32, dict(quality=20)),
             ("L", "noise", 32, dict(quality=90)),
             ("L", "noise", 32, dict(quality=100)),
             ("L", "noise", 32, dict(quality=90, optimize=True)),
             ("L", "smooth", 48, dict(quality=90)),
             ("L", "smooth", 32, dict(quality=75, restart_marker_blocks=1)),
             ("L", "smooth", 32, dict(qtables=[[255] * 64])),
             ("L", "noise", 32, dict(quality=50, optimize=True, restart_marker_blocks=2))],
    "four": [("4", "smooth", 32, dict(quality=30)),
             ("4", "noise", 32, dict(quality=90)),
             ("4", "noise", 32, dict(quality=100)),
             ("4", "noise", 32, dict(quality=90, optimize=True)),
             ("4", "smooth", 48, dict(quality=90)),
             ("4", "smooth", 32, dict(quality=90, restart_marker_blocks=3)),
             ("4", "smooth", 32, dict(quality=30, optimize=True)),
             ("4", "smooth", 32, dict(quality=75, restart_marker_blocks=1))],
}


def mixed(variant: str) -> Case:
    blocks = []
    for k, (mode, kind, rows, kw) in enumerate(MIXED[variant]):
        img = image4(rows, 48, kind, seed=40 + k) if mode == "4" else image(rows, 48, kind, seed=40 + k)
        blocks.append(encode(img, mode, **kw))
    blocks.append(blocks[0])
    return make_case(f"mixed-{variant}", blocks, 3, 48, 32, 131, 85, {"rgb": 3, "grey": 1, "four": 4}[variant])


# 2. tiny: one-block rasters of a few pixels (block = raster): components of 1 - 2 samples, replicated chroma, single rows and columns.
def tiny(size, mode: str) -> Case:
    h, w = size
    stream = encode(image(h, w, "noise", seed=h * 7 + w), mode, quality=85)
    return make_case(f"tiny-{h}x{w}-{mode}", [stream], 1, w, h, w, h, 1 if mode == "L" else 3)


# 3. restage: many one-MCU, one-segment 4:2:0 blocks of 16 x 16 drawn from P streams of pairwise distinct table sets — more long
# segments than the wave launch has waves, so that a wave takes a second segment, of another set.
RESTAGE_STANDARD = [25, 40, 55, 70, 85, 95]                    # standard Huffman tables: the sets differ by the quantisation tables alone
RESTAGE_OPTIMIZED = [30, 50, 75, 90]                           # optimize=True: Huffman tables of their own as well


def _restage_image(seed: int) -> np.ndarray:
    """16 x 16 around mid-grey with a small texture: coefficients small enough that every pool stream still decodes WITHOUT error
    under any other pool stream's quantisation tables (the decoder refuses a coefficient whose product leaves the sample range):
    the first control of test_jpeg_cases.py splices them and requires other pixels without an error. The price: a stale LDS set in
    the wave kernel, which serves that range check and the Huffman tables alone, shows only where the Huffman tables change."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:16, :16]
    base = np.stack([128 + 6 * np.sin(xx / 3.0 + c + seed) * np.cos(yy / 2.5) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 1.5, base.shape), 0, 255).astype(np.uint8)


def restage_pool() -> List[bytes]:
    pool = [encode(_restage_image(100 + q), "420", quality=q) for q in RESTAGE_STANDARD]
    pool += [encode(_restage_image(200 + q), "420", quality=q, optimize=True) for q in RESTAGE_OPTIMIZED]
    assert len(pool) == POOL_SIZE
    return pool


def restage_block_count(cus: int, across: int = 32) -> int:
    n = 4 * cus + 256
    return -(-n // across) * across


def restage_waves(nseg: int, cus: int) -> int:
    """The waves td_tiff_jpeg_decode_long_dev launches for nseg long segments: min(ceil(n / 4), CUs) workgroups of 4."""
    return min(-(-nseg // 4), cus) * 4


def restage(cus: int):
    """→ (case, draw): draw[b] = the pool stream of block b. The raster crops 3 columns and 5 rows of the last blocks."""
    across = 32
    n = restage_block_count(cus, across)
    pool = restage_pool()
    draw = np.random.default_rng(77).integers(0, POOL_SIZE, n)
    refs = [pillow(s) for s in pool]
    case = make_case(f"restage-{n}", [pool[i] for i in draw], across, 16, 16, across * 16 - 3, n // across * 16 - 5, 3,
                     refs=[refs[i] for i in draw])
    return case, draw


def header_segments(stream: bytes, marker: int):
    """(position, length with the marker) of every segment of `marker` before SOS."""
    out, pos = [], 2
    while stream[pos + 1] != 0xDA:
        n = (stream[pos + 2] << 8) | stream[pos + 3]
        if stream[pos + 1] == marker:
            out.append((pos, 2 + n))
        pos += 2 + n
    return out


def splice_dqt(stream: bytes, donor: bytes) -> bytes:
    """stream with donor's DQT segments in place of its own (the same lengths: a byte splice)."""
    mine, theirs = header_segments(stream, 0xDB), header_segments(donor, 0xDB)
    assert len(mine) == len(theirs) > 0 and all(a[1] == b[1] for a, b in zip(mine, theirs))
    data = bytearray(stream)
    for (p, n), (q, _) in zip(mine, theirs):
        data[p:p + n] = donor[q:q + n]
    return bytes(data)


def dht_bytes(stream: bytes) -> bytes:
    """The stream's DHT segments, one after the other."""
    return b"".join(stream[p:p + n] for p, n in header_segments(stream, 0xC4))


def splice_dht(stream: bytes, donor: bytes) -> bytes:
    """stream with donor's DHT segments where its own first one stood (optimised tables differ in length: the header is rebuilt)."""
    mine = header_segments(stream, 0xC4)
    assert mine and header_segments(donor, 0xC4)
    out, pos = bytearray(), 0
    for k, (p, n) in enumerate(mine):
        out += stream[pos:p]
        if k == 0:
            out += dht_bytes(donor)
        pos = p + n
    return bytes(out + stream[pos:])


# 4. wave_counts. (a) 63 / 64 / 65 blocks of a component in one segment (the DC scan's carry across 64-block steps); 64 chroma and 256
# luma blocks. (b) one stream cut into exactly 1 / 2 / 63 / 64 / 65 / 128 / 129 subsequences (L, valid and carry at the window's edge).
def wave_dc(name: str) -> Case:
    if name == "420-128x128":
        return make_case("wave-" + name, [encode(image(128, 128, "smooth", seed=8), "420", quality=90)], 1, 128, 128, 128, 128, 3)
    cols = 8 * int(name.split("-")[1])
    return make_case("wave-" + name, [encode(image(8, cols, "smooth", seed=cols), "L", quality=90)], 1, cols, 8, cols, 8, 1)


# ceil(n / S) == 128 and == 129 for two sizes S need n > 127 * 65 bytes: the 96 x 64 stream's ~5.5 KB segment has no size for 128
# (5 540 bytes: S = 43 gives 129, S = 44 gives 126), so it takes the other six targets and a 128 x 96 stream of the same kind (~11 KB,
# seed chosen so that every target has a size: wave_subseq asserts it) takes all seven.
WAVE_STREAMS = {"96x64": (64, 96, 0, [1, 2, 63, 64, 65, 129]), "128x96": (96, 128, 3, WAVE_TARGETS)}
WAVE_CASES = [(name, t) for name, v in WAVE_STREAMS.items() for t in v[3]]


_WAVE_CACHE = {}


def wave_stream(name: str) -> Case:
    """The stream of the listed seed. Should another libjpeg build encode it to a byte count that misses a target, wave_subseq says so."""
    if name not in _WAVE_CACHE:
        h, w, seed, _ = WAVE_STREAMS[name]
        _WAVE_CACHE[name] = make_case("wave-" + name, [encode(image(h, w, "smooth", seed=seed), "444", quality=90)], 1, w, h, w, h, 3)
    return _WAVE_CACHE[name]


def subsequences(nbytes: int, subseq: int) -> int:
    """How many subsequences a segment of nbytes is cut into (jpeg_core.h: one when it fits)."""
    return -(-nbytes // subseq) if nbytes > subseq else 1


def wave_subseq(nbytes: int, target: int) -> int:
    """The smallest subsequence size in 4 .. 2^20 that cuts nbytes into exactly `target` subsequences."""
    for s in range(4, (1 << 20) + 1):
        k = subsequences(nbytes, s)
        if k == target:
            return s
        if k < target:
            break
    raise AssertionError(f"no subsequence size cuts {nbytes} bytes into {target}: choose another seed")


# 5. flips: every 5th bit of the entropy-coded data of three 48 x 32 streams, each flipped stream one block of a one-row raster.
def flip_stream(name: str) -> bytes:
    if name == "420-q90-smooth":
        return encode(image(32, 48, "smooth", seed=61), "420", quality=90)
    if name == "422-q75-restart2":
        return encode(image(32, 48, "smooth", seed=62), "422", quality=75, restart_marker_blocks=2)
    assert name == "444-q60-optimize"
    return encode(image(32, 48, "smooth", seed=63), "444", quality=60, optimize=True)


def flipped(stream: bytes) -> List[bytes]:
    e0, e1 = entropy_span(stream)
    out = []
    for bit in range(0, 8 * (e1 - e0), FLIP_STRIDE):
        bad = bytearray(stream)
        bad[e0 + (bit >> 3)] ^= 0x80 >> (bit & 7)
        out.append(bytes(bad))
    return out


@dataclass
class Flips:
    case: Case                                 # the launch: the original stream, the accepted flipped streams, the original stream
    expect_status: np.ndarray                  # per block of the launch
    streams: List[bytes] = field(repr=False)   # EVERY flipped stream, the refused ones included
    outcomes: list = field(repr=False)         # td_jpeg_decode of each: [h, w, c] uint8, or the negative error code
    refused: np.ndarray = field(repr=False)    # per flipped stream: td_tiff_jpeg_plan marks it unsupported (left out of the launch only)

    @property
    def total(self) -> int:
        return len(self.streams)

    @property
    def host_errors(self) -> int:
        return sum(isinstance(o, int) for o in self.outcomes)


def flips(name: str) -> Flips:
    """The expected outcome is the host twin's: td_jpeg_decode < 0 → status 1 and the pixels are not compared, otherwise status 0 and
    the host's bytes. A stream the plan refuses (a forged or broken marker) is a host-side refusal and stays out of the launch."""
    stream = flip_stream(name)
    cases = flipped(stream)
    outcome = [host_decode(s) for s in cases]
    probe = Case("probe", cases, len(cases), 48, 32, 48 * len(cases), 32, 3)
    info = plan(probe, allow_unsupported=True).info
    refused = info[:, 0] != 0
    good = host_decode(stream)
    assert not isinstance(good, int) and np.array_equal(good, pillow(stream))
    blocks, refs, status = [stream], [good], [0]
    for s, o, r in zip(cases, outcome, refused):
        if r:
            continue
        blocks.append(s)
        refs.append(None if isinstance(o, int) else o)
        status.append(1 if isinstance(o, int) else 0)
    blocks.append(stream)
    refs.append(good)
    status.append(0)
    case = make_case(f"flips-{name}", blocks, len(blocks), 48, 32, 48 * len(blocks), 32, 3, refs=refs)
    return Flips(case, np.array(status, dtype=np.int32), cases, outcome, refused)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Plan:
    data: np.ndarray                           # the blocks in one buffer: 1 - 3 bytes before each (odd offsets), 16 zero bytes behind
    offs: np.ndarray
    info: np.ndarray                           # [nblocks, 8]
    segs: np.ndarray                           # [nseg, 4]
    sets: np.ndarray                           # [nsets, TD_JPEG_TABSET_BYTES]
    ncoef: int
    unsupported: int


def plan(case: Case, allow_unsupported: bool = False) -> Plan:
    """td_tiff_jpeg_plan on the case's blocks: no JPEGTables, photometric 6. Must return TD_OK (and no unsupported block, unless allowed)."""
    lib = _lib.load()
    parts, offs, pos = [], [], 0
    for k, s in enumerate(case.blocks):
        pad = 1 + k % 3
        if (pos + pad) % 2 == 0:
            pad += 1 if pad < 3 else -1
        parts.append(bytes([0xA0 + pad]) * pad)
        offs.append(pos + pad)
        parts.append(s)
        pos += pad + len(s)
    data = np.frombuffer(b"".join(parts) + bytes(16), dtype=np.uint8).copy()
    offs = np.array(offs, dtype=np.int64)
    assert (offs % 2 == 1).all()
    cnts = np.array([len(s) for s in case.blocks], dtype=np.int64)
    rows = case.block_rows()
    nb = len(case.blocks)
    info, totals = np.zeros((nb, 8), dtype=np.int64), np.zeros(4, dtype=np.int64)
    segs, sets = np.zeros((nb, 4), dtype=np.int64), np.zeros((4, _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
    tables = np.zeros(1, dtype=np.uint8)
    for _ in range(2):
        st = lib.td_tiff_jpeg_plan(tables.ctypes.data, 0, data.ctypes.data, offs.ctypes.data, cnts.ctypes.data, nb, 6, case.bands, case.bw,
                                   rows.ctypes.data, info.ctypes.data, segs.ctypes.data, len(segs), sets.ctypes.data, len(sets),
                                   totals.ctypes.data)
        if st != _lib.ERR_CAPACITY:
            break
        segs = np.zeros((int(totals[0]), 4), dtype=np.int64)
        sets = np.zeros((int(totals[1]), _lib.JPEG_TABSET_BYTES), dtype=np.uint8)
    assert st == 0, (case.name, st, lib.td_last_error())
    assert allow_unsupported or int(totals[3]) == 0, (case.name, int(totals[3]))
    return Plan(data, offs, info, segs[:int(totals[0])], sets[:int(totals[1])], int(totals[2]), int(totals[3]))


# ---- the device ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Result:
    image: np.ndarray                          # [height, width, bands]
    status: np.ndarray                         # [nblocks]
    stats: Optional[List[int]]                 # the wave decoder's four counts, None for the lane-per-segment entry
    canaries: bool                             # every canary on either side of coef, planes, status, stats and image survived
    long_segments: int = 0
    earlier: list = field(default_factory=list)    # (image, status, stats) of the runs before the last (runs > 1)


CANARY = {"coef": 0x5A5A, "planes": 0xA5, "status": 0x5A5A5A5A, "stats": 0x5A5A5A5A5A5A5A5A, "image": 0xA5}


class Device:
    """A case's plan uploaded, and coef / planes / status / stats / image inside canary-filled buffers (GUARD elements either side;
    the insides start as canaries too). launch() calls an entry point on the current stream, fetch() waits and reads everything back."""

    def __init__(self, case: Case, pl: Optional[Plan] = None):
        import torch
        self.torch = torch
        self.case, self.plan = case, pl or plan(case)
        pl = self.plan
        assert pl.unsupported == 0
        self.comp = torch.from_numpy(pl.data).cuda()
        self.info = torch.from_numpy(pl.info).cuda()
        self.sets = torch.from_numpy(pl.sets).cuda()
        self.segs = torch.from_numpy(pl.segs).cuda()
        self.nlong = 0
        dtypes = {"coef": torch.int16, "planes": torch.uint8, "status": torch.int32, "stats": torch.int64, "image": torch.uint8}
        self.sizes = {"coef": max(pl.ncoef, 64), "planes": max(pl.ncoef, 64), "status": len(case.blocks), "stats": 4,
                      "image": case.height * case.width * case.bands}
        self.bufs = {k: torch.full((GUARD + n + GUARD,), CANARY[k], dtype=dtypes[k], device="cuda") for k, n in self.sizes.items()}

    def ptr(self, name: str) -> int:
        b = self.bufs[name]
        return b.data_ptr() + GUARD * b.element_size()

    def grid(self):
        c = self.case
        return [c.width, c.height, c.bands, c.bw, c.bh, c.across]

    def args_dev(self) -> list:
        """td_tiff_jpeg_decode_dev's arguments, in order."""
        pl = self.plan
        return [self.comp.data_ptr(), self.info.data_ptr(), len(self.case.blocks), self.segs.data_ptr(), len(pl.segs), self.sets.data_ptr(),
                self.ptr("coef"), self.ptr("planes"), pl.ncoef, self.ptr("status"), self.ptr("image"), *self.grid(), _lib.stream_ptr()]

    def args_long(self, long_threshold: int, subseq_bytes: Optional[int] = None) -> list:
        """td_tiff_jpeg_decode_long_dev's arguments, the segments split as GeoTiff._jpeg_to_device splits them: one upload, the short
        ones first, the long ones (more than long_threshold bytes) behind them, each list in the plan's order."""
        pl, torch = self.plan, self.torch
        is_long = pl.segs[:, 1] > int(long_threshold)
        self.nlong = nlong = int(is_long.sum())
        nshort = len(pl.segs) - nlong
        self.segs_split = torch.from_numpy(np.concatenate([pl.segs[~is_long], pl.segs[is_long]])).cuda()
        return [self.comp.data_ptr(), self.info.data_ptr(), len(self.case.blocks), self.segs_split.data_ptr() if nshort else None, nshort,
                self.segs_split[nshort:].data_ptr() if nlong else None, nlong, int(subseq_bytes or DEFAULT_SUBSEQ), self.sets.data_ptr(),
                self.ptr("coef"), self.ptr("planes"), pl.ncoef, self.ptr("status"), self.ptr("stats"), self.ptr("image"), *self.grid(),
                _lib.stream_ptr()]

    def untouched(self) -> bool:
        """Every buffer still holds nothing but canaries, inside and out (an entry point that refused has launched nothing)."""
        self.torch.cuda.synchronize()
        return all(bool((b == CANARY[k]).all()) for k, b in self.bufs.items())

    def fetch(self, with_stats: bool):
        self.torch.cuda.synchronize()
        host = {k: b.cpu().numpy() for k, b in self.bufs.items()}
        alive = True
        for k, a in host.items():
            if k == "stats" and not with_stats:
                alive &= bool((a == CANARY[k]).all())
                continue
            alive &= bool((a[:GUARD] == CANARY[k]).all() and (a[GUARD + self.sizes[k]:] == CANARY[k]).all())
        c = self.case
        img = host["image"][GUARD:GUARD + self.sizes["image"]].reshape(c.height, c.width, c.bands).copy()
        status = host["status"][GUARD:GUARD + self.sizes["status"]].copy()
        stats = [int(v) for v in host["stats"][GUARD:GUARD + 4]] if with_stats else None
        return img, status, stats, alive


def decode_on_device(case: Case, long_threshold: Optional[int] = None, subseq_bytes: Optional[int] = None, runs: int = 1,
                     pl: Optional[Plan] = None) -> Result:
    """The case through td_tiff_jpeg_decode_dev, or (long_threshold given) through td_tiff_jpeg_decode_long_dev. runs > 1: the same launch
    again on the same buffers; the earlier runs' outcomes are kept in Result.earlier."""
    lib = _lib.load()
    d = Device(case, pl)
    outcomes, alive = [], True
    for _ in range(runs):
        if long_threshold is None:
            _lib.check(lib.td_tiff_jpeg_decode_dev(*d.args_dev()), "td_tiff_jpeg_decode_dev")
        else:
            _lib.check(lib.td_tiff_jpeg_decode_long_dev(*d.args_long(long_threshold, subseq_bytes)), "td_tiff_jpeg_decode_long_dev")
        img, status, stats, ok = d.fetch(long_threshold is not None)
        alive &= ok
        outcomes.append((img, status, stats))
    img, status, stats = outcomes[-1]
    return Result(img, status, stats, alive, d.nlong, outcomes[:-1])


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
def check(case: Case, result: Result, expect_status=None) -> None:
    """Status per block (default: all 0), the image byte for byte on every block whose expected status is 0, the canaries."""
    nb = len(case.blocks)
    want = np.zeros(nb, dtype=np.int32) if expect_status is None else np.asarray(expect_status, dtype=np.int32)
    assert result.canaries, f"{case.name}: a canary beside a device buffer was overwritten"
    assert result.status.shape == (nb,) and want.shape == (nb,)
    wrong = np.nonzero(result.status != want)[0]
    assert wrong.size == 0, f"{case.name}: status of block {int(wrong[0])} is {int(result.status[wrong[0]])}, expected {int(want[wrong[0]])} ({wrong.size} blocks differ)"
    assert result.image.shape == case.expected.shape and result.image.dtype == np.uint8
    differ = result.image != case.expected
    for b in np.nonzero(want == 0)[0]:
        y0, x0, rows, cols = case.rect(int(b))
        n = int(differ[y0:y0 + rows, x0:x0 + cols].sum())
        assert n == 0, f"{case.name}: block {int(b)} at ({y0}, {x0}) differs in {n} bytes"
