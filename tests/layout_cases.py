"""What the pixel-interleaved (chunky) layout kernels of tiffdecode.hip must compute, in plain numpy, and the tables of cases that
tests/test_layout_kernels_gpu.py feeds them: td_tiff_blocks_to_image_dev / _u16_dev / _f32_dev take the block decoder's bytes
(blocks_across x blocks_down blocks of bh x bw pixels, each at a multiple of block_cap bytes), undo the predictor per block row and
write [height][width][spp]. Nothing here calls the library; tests/test_layout_cases.py pins the oracle to the host twins
(td_tiff_unpredict, td_tiff_unpredict_float) and shows that every entry of DEFECTS — what a subtly wrong kernel would compute —
changes the expected bytes of a case of the tables."""
import numpy as np

ENTRY = {1: "td_tiff_blocks_to_image_dev", 2: "td_tiff_blocks_to_image_u16_dev", 4: "td_tiff_blocks_to_image_f32_dev"}
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}          # uint32: the bit patterns of float32 samples
KERNEL_CASES = [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3)]      # (bytes per sample, predictor)
# below a dword and a wave, around the RGBI kernel's 64-pixel step, around the generic kernel's 256 threads (from 257 on a thread's run
# is two pixels and more) and predictor 3's 256-position step, carries across several steps
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
HEIGHTS_BH = (1, 3, 4)
PADS = {1: (0, 3, 8), 2: (0, 6), 4: (0, 12)}               # bytes of capacity behind a block; uint8 / uint16: one that is no multiple of 4
CRAFTED_WIDTHS = (65, 257, 513, 1025)
LONG_WIDTH = 20011                                          # 79-pixel runs, 313 steps of 64 pixels, byte planes that begin at odd bytes


def kernel_of(item, spp, predictor, cap, blocks_shift=0, image_shift=0):
    """Which kernel blocks_to_image launches: 'rgbi' (uint8, four bands, blocks, image and block_cap multiples of 4), 'plane' (predictor
    3) or 'generic'."""
    if item == 1 and spp == 4 and cap % 4 == 0 and blocks_shift % 4 == 0 and image_shift % 4 == 0:
        return "rgbi"
    return "plane" if predictor == 3 else "generic"


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
def fp_byte_sums(rows, spp):
    """Predictor 3, first half: [bh, 4n] difference bytes → the running sums modulo 256 with stride spp over all 4n bytes of a row."""
    return np.cumsum(rows.reshape(rows.shape[0], -1, spp), axis=1, dtype=np.uint8).reshape(rows.shape)


def fp_assemble(sums, n):
    """Predictor 3, second half: float k of a row is the bytes (r[k], r[n + k], r[2n + k], r[3n + k]), most significant first."""
    p = sums.reshape(sums.shape[0], 4, n).astype(np.uint32)
    return (p[:, 0] << 24) | (p[:, 1] << 16) | (p[:, 2] << 8) | p[:, 3]


def unpredict(block, item, bw, bh, spp, predictor):
    """The bw * bh * spp * item bytes of one block → its samples [bh, bw, spp] of DTYPE[item]."""
    if predictor == 3:
        return fp_assemble(fp_byte_sums(block.reshape(bh, 4 * bw * spp), spp), bw * spp).reshape(bh, bw, spp)
    samples = block.view(DTYPE[item]).reshape(bh, bw, spp)
    return np.cumsum(samples, axis=1, dtype=DTYPE[item]) if predictor == 2 else samples.copy()


def oracle(blocks, item, bw, bh, nx, ny, spp, predictor, width, height):
    """blocks [nx * ny, cap] uint8 → the raster [height, width, spp] of DTYPE[item]. The bytes behind bw * bh * spp * item of a block are
    capacity, not data; of each block only the part inside the raster lands in it."""
    out = np.zeros((height, width, spp), dtype=DTYPE[item])
    for by in range(ny):
        for bx in range(nx):
            blk = unpredict(np.array(blocks[by * nx + bx, :bw * bh * spp * item]), item, bw, bh, spp, predictor)
            y0, x0 = by * bh, bx * bw
            rows, cols = min(bh, height - y0), min(bw, width - x0)
            out[y0:y0 + rows, x0:x0 + cols] = blk[:rows, :cols]
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def geometry(bw, bh, keep):
    """→ (nx, ny, width, height): two or three block columns of which the last keeps `keep` pixels, two block rows of which the second
    keeps the upper half (for bh = 3 the raster is 5 rows: the RGBI kernel's second group of four rows is cut after one)."""
    nx, ny = (3 if bw < 300 else 2), 2
    return nx, ny, (nx - 1) * bw + keep, bh + (bh + 1) // 2


def random_blocks(rng, count, cap):
    """Uniform bytes, the capacity padding included: padding PIXELS of an edge block are not zero and take part in the sums."""
    return rng.integers(0, 256, (count, cap), dtype=np.uint8)


def crafted_rows(item, spp, bw, predictor=2):
    """[2, bw * spp * item] bytes, two block rows that pin the carry itself. Row 0: the first pixel is a non-zero constant (another per
    band) and every difference is 0, so every pixel must equal the first — a carry that is lost anywhere shows as a 0. Row 1: every
    difference byte is 0xFF, so every sum wraps at every step. Predictor 3 differences bytes: there the constant is the first spp
    BYTES of the 4n."""
    rows = np.zeros((2, bw * spp * item), dtype=np.uint8)
    if predictor == 3:
        rows[0, :spp] = 0xA1 + np.arange(spp)
    else:
        first = np.array([{1: 0xA1, 2: 0xA1B2, 4: 0xA1B2C3D4}[item] + c for c in range(spp)], dtype=DTYPE[item])
        rows[0, :spp * item] = first.view(np.uint8)
    rows[1] = 0xFF
    return rows


def sweep(item):
    """The (spp, bw, bh, pad, keep) of test_every_entry_equals_numpy_at_every_block_width, in launch order: every band count at every
    width, then every (bh, pad, keep) at every width with the band count rotating so that each combination meets each band count at
    three widths or more."""
    for bw in WIDTHS:
        for spp in (1, 2, 3, 4):
            yield spp, bw, 3, 0, bw
    for i, bw in enumerate(WIDTHS):
        j = 0
        for bh in HEIGHTS_BH:
            for pad in PADS[item]:
                for keep in (1, bw):
                    yield 1 + (i + j) % 4, bw, bh, pad, keep
                    j += 1


def sweep_seed(item, predictor):
    return 100 * item + predictor


def sweep_inputs(item, predictor):
    """→ ((spp, bw, bh, pad, keep), (nx, ny, width, height), cap, blocks) per case of sweep(item), the blocks drawn in order from ONE
    generator per (item, predictor): the GPU test and the CPU test of the defects see the same bytes."""
    rng = np.random.default_rng(sweep_seed(item, predictor))
    for spp, bw, bh, pad, keep in sweep(item):
        geom = geometry(bw, bh, keep)
        cap = bw * bh * spp * item + pad
        yield (spp, bw, bh, pad, keep), geom, cap, random_blocks(rng, geom[0] * geom[1], cap)


# ---- what a subtly wrong kernel would compute ---------------------------------------------------------------------------------------------
def _restarting_cumsum(samples, every, dtype):
    out = np.empty_like(samples)
    for a in range(0, samples.shape[1], every):
        out[:, a:a + every] = np.cumsum(samples[:, a:a + every], axis=1, dtype=dtype)
    return out


def _fp_restarting(rows, spp, n, every):
    """Stride-spp byte sums that keep the carry from plane to plane but lose it every `every` positions inside a plane."""
    d = rows.reshape(rows.shape[0], 4, n).astype(np.int64)
    out = np.empty_like(d)
    for c in range(spp):
        dc = d[:, :, c::spp]                                # channel c: positions c, c + spp, … of every plane
        pos = np.arange(c, n, spp)
        _, first, inverse = np.unique(pos // every, return_index=True, return_inverse=True)
        run = np.cumsum(dc, axis=2)
        run = run - (run[:, :, first] - dc[:, :, first])[:, :, inverse]
        total = dc.sum(axis=2)
        out[:, :, c::spp] = run + (np.cumsum(total, axis=1) - total)[:, :, None]
    return (out & 255).astype(np.uint8).reshape(rows.shape)


def _fp_phase_zero(rows, n):
    """Three bands, every dword of a plane taken to begin at channel 0: a byte's running sum is kept per (position % 4) % 3 instead of
    per position % 3 — inside the dword byte 3 still adds byte 0, across dwords, steps and planes the totals land in the wrong band."""
    m = -(-n // 4) * 4
    d = np.zeros((rows.shape[0], 4, m), dtype=np.int64)
    d[:, :, :n] = rows.reshape(rows.shape[0], 4, n)
    d = d.reshape(rows.shape[0], 4 * m // 4, 4)             # [row, dword (plane after plane), byte]
    slot = np.stack([d[:, :, 0] + d[:, :, 3], d[:, :, 1], d[:, :, 2]], axis=2)
    before = np.cumsum(slot, axis=1) - slot
    out = d + before[:, :, [0, 1, 2, 0]]
    out[:, :, 3] += d[:, :, 0]
    return (out & 255).astype(np.uint8).reshape(rows.shape[0], 4, m)[:, :, :n].reshape(rows.shape)


def _faulty_unpredict(name, block, item, bw, bh, spp, predictor):
    dtype, n = DTYPE[item], bw * spp
    if predictor == 2:
        samples = block.view(dtype).reshape(bh, bw, spp)
        if name == "carry_lost_at_64":
            return _restarting_cumsum(samples, 64, dtype)
        if name == "carry_lost_at_run":
            return _restarting_cumsum(samples, -(-bw // 256), dtype)
        if name == "saturating_add":
            return np.minimum(np.cumsum(samples, axis=1, dtype=np.uint64), np.iinfo(dtype).max).astype(dtype)
        if name == "stride_one_for_spp":
            return np.cumsum(samples.reshape(bh, n), axis=1, dtype=dtype).reshape(bh, bw, spp)
    if predictor == 3:
        rows = block.reshape(bh, 4 * n)
        sums = None
        if name == "carry_lost_at_256_bytes":
            sums = _fp_restarting(rows, spp, n, 256)
        if name == "saturating_add":
            sums = np.minimum(np.cumsum(rows.reshape(bh, -1, spp), axis=1, dtype=np.uint64), 255).astype(np.uint8).reshape(bh, 4 * n)
        if name == "stride_one_for_spp":
            sums = np.cumsum(rows, axis=1, dtype=np.uint8)
        if name == "plane_carry_dropped":
            sums = np.cumsum(rows.reshape(bh, 4, bw, spp), axis=2, dtype=np.uint8).reshape(bh, 4 * n)
        if name == "phase_zero_for_three_bands" and spp == 3:
            sums = _fp_phase_zero(rows, n)
        if sums is not None:
            return fp_assemble(sums, n).reshape(bh, bw, spp)
    return unpredict(block, item, bw, bh, spp, predictor)


class Defect:
    """A faulty variant of oracle(), called like it. ``predictors``: where it differs from the oracle at all."""

    def __init__(self, name, predictors, what):
        self.name, self.predictors, self.what = name, predictors, what

    def __call__(self, blocks, item, bw, bh, nx, ny, spp, predictor, width, height):
        out = np.zeros((height, width, spp), dtype=DTYPE[item])
        flat = out.reshape(-1)
        spill = []
        for by in range(ny):
            for bx in range(nx):
                blk = _faulty_unpredict(self.name, np.array(blocks[by * nx + bx, :bw * bh * spp * item]), item, bw, bh, spp, predictor)
                y0, x0 = by * bh, bx * bw
                rows, cols = min(bh, height - y0), min(bw, width - x0)
                out[y0:y0 + rows, x0:x0 + cols] = blk[:rows, :cols]
                if self.name == "edge_block_full_width":
                    spill += [(((y0 + r) * width + x0 + cols) * spp, blk[r, cols:].reshape(-1)) for r in range(rows)]
        for at, samples in spill:                           # taken to land last; what falls behind the raster is the guard's to show
            flat[at:at + samples.size] = samples[:max(0, flat.size - at)]
        return out


DEFECTS = {d.name: d for d in (
    Defect("carry_lost_at_64", (2,), "the running sum restarts every 64 pixels (the RGBI kernel's step)"),
    Defect("carry_lost_at_run", (2,), "it restarts at every thread-run boundary of the generic kernel, ceil(bw / 256) pixels"),
    Defect("carry_lost_at_256_bytes", (3,), "predictor 3: it restarts every 256 positions of a byte plane"),
    Defect("saturating_add", (2, 3), "clamps instead of wrapping"),
    Defect("stride_one_for_spp", (2, 3), "sums neighbouring samples instead of the same band's"),
    Defect("plane_carry_dropped", (3,), "predictor 3: a byte plane starts from 0 instead of the totals of the planes before it"),
    Defect("phase_zero_for_three_bands", (3,), "predictor 3, three bands: every dword taken to begin at channel 0"),
    Defect("edge_block_full_width", (1, 2, 3), "an edge block writes bw pixels where only `valid` lie inside the raster"),
)}
