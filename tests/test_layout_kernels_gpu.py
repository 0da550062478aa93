"""The pixel-interleaved (chunky) layout kernels of tiffdecode.hip alone, through td_tiff_blocks_to_image_dev / _u16_dev / _f32_dev,
against the numpy oracle of tests/layout_cases.py, byte for byte: random blocks at every width around a dword, a wave, the RGBI
kernel's 64-pixel step, the generic kernel's 256 runs and predictor 3's 256-position step; padded capacities, partial edge blocks,
row groups cut by the height, buffers off their alignment; crafted rows that pin the carry; 4096-byte guards around the raster. No
tolerance anywhere. tests/test_layout_cases.py pins the oracle to the host twins and shows which case catches which faulty kernel."""
import numpy as np
import pytest
import torch

import layout_cases as lc
from treedetection_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 4096


def run(rng, item, spp, bw, bh, pad, keep, predictor, blocks_shift=0, image_shift=0, blocks=None, geom=None):
    """One launch → (got, want) as byte arrays. ``pad``: bytes of capacity behind a block; ``keep``: pixels of the last block column
    inside the raster (``geom`` = (nx, ny, width, height) in place of layout_cases.geometry); ``blocks_shift`` / ``image_shift``: bytes by
    which a buffer is moved off its alignment; ``blocks`` [nx * ny, cap] in place of random ones. The image lies between guards,
    everything filled with 0xFF beforehand; both guards must still hold it afterwards."""
    nx, ny, width, height = geom or lc.geometry(bw, bh, keep)
    cap = bw * bh * spp * item + pad
    if blocks is None:
        blocks = lc.random_blocks(rng, nx * ny, cap)
    assert blocks.shape == (nx * ny, cap) and blocks.dtype == np.uint8
    d_buf = torch.empty((blocks.size + 16,), dtype=torch.uint8, device="cuda")
    d_blocks = d_buf[blocks_shift:blocks_shift + blocks.size]
    d_blocks.copy_(torch.from_numpy(np.ascontiguousarray(blocks).reshape(-1)))
    nbytes = width * height * spp * item
    d_image = torch.full((GUARD + nbytes + GUARD + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 16 == 0 and d_image.data_ptr() % 16 == 0
    at = GUARD + image_shift
    st = getattr(_lib.load(), lc.ENTRY[item])(d_blocks.data_ptr(), cap, bw, bh, nx, ny, spp, predictor, d_image.data_ptr() + at, width, height,
                                              _lib.stream_ptr())
    _lib.check(st, lc.ENTRY[item])
    torch.cuda.synchronize()
    got = d_image.cpu().numpy()
    assert (got[:at] == 0xFF).all() and (got[at + nbytes:] == 0xFF).all(), "a store outside the image"
    want = lc.oracle(blocks, item, bw, bh, nx, ny, spp, predictor, width, height)
    return got[at:at + nbytes], want.reshape(-1).view(np.uint8)


@pytest.mark.parametrize("item,predictor", lc.KERNEL_CASES)
def test_every_entry_equals_numpy_at_every_block_width(item, predictor):
    """layout_cases.sweep: bands 1 - 4 at every width (bh = 3, exact capacity, whole edge blocks), then every block height, capacity
    padding and edge-block width at every width with the band count rotating. Which kernel a launch takes: uint8 with four bands and a
    capacity that is a multiple of 4 takes tiff_blocks_to_image_rgbi_kernel (pad 0 and 8; pad 3 sends the same shape to the generic
    <uint8_t, 4>); float32 with predictor 3 takes tiff_fp_blocks_to_image_kernel<spp>; everything else takes
    tiff_blocks_to_image_kernel<T, spp>."""
    for (spp, bw, bh, pad, keep), geom, cap, blocks in lc.sweep_inputs(item, predictor):
        got, want = run(None, item, spp, bw, bh, pad, keep, predictor, blocks=blocks)
        assert np.array_equal(got, want), (lc.kernel_of(item, spp, predictor, cap), spp, bw, bh, pad, keep)


@pytest.mark.parametrize("item,predictor", lc.KERNEL_CASES)
def test_crafted_carries(item, predictor):
    """One block of two rows: a constant first pixel with every difference 0 (a carry dropped anywhere leaves a 0), and every
    difference byte 0xFF (every sum wraps at every step)."""
    for bw in lc.CRAFTED_WIDTHS:
        for spp in (1, 2, 3, 4):
            rows = lc.crafted_rows(item, spp, bw, predictor)
            got, want = run(None, item, spp, bw, 2, 0, bw, predictor, blocks=rows.reshape(1, -1), geom=(1, 1, bw, 2))
            assert np.array_equal(got, want), (spp, bw)


@pytest.mark.parametrize("item,predictor", lc.KERNEL_CASES)
def test_rows_far_longer_than_one_step(item, predictor):
    """Strips of one row, 20 011 pixels wide, three of them: 79-pixel runs per thread in the generic kernel, 313 steps of 64 pixels in the
    RGBI kernel, up to 313 steps of 256 positions and byte planes that begin at odd bytes (20 011 x spp is odd for spp 1 and 3) under
    predictor 3. Random rows, then the constant row between two wrapping ones."""
    rng = np.random.default_rng(300 * item + predictor)
    bw = lc.LONG_WIDTH
    for spp in (1, 2, 3, 4):
        got, want = run(rng, item, spp, bw, 1, 0, bw, predictor, geom=(1, 3, bw, 3))
        assert np.array_equal(got, want), spp
        if item == 1 and spp == 4:                          # three bytes of capacity: the generic <uint8_t, 4> in place of the wave kernel
            got, want = run(rng, item, spp, bw, 1, 3, bw, predictor, geom=(1, 3, bw, 3))
            assert np.array_equal(got, want), "generic"
        rows = lc.crafted_rows(item, spp, bw, predictor)
        got, want = run(None, item, spp, bw, 1, 0, bw, predictor, blocks=rows[[1, 0, 1]], geom=(1, 3, bw, 3))
        assert np.array_equal(got, want), spp


@pytest.mark.parametrize("predictor", [1, 2])
def test_four_band_uint8_off_its_alignment_equals_the_wave_kernel(predictor):
    """uint8 x 4 takes the wave kernel only when blocks, image and block_cap are multiples of 4; otherwise the launcher falls back to
    the generic <uint8_t, 4>. The same blocks through the aligned launch, with the block buffer moved by 1, 2 and 3 bytes, with 1, 2 and
    3 bytes of capacity behind every block, and with the image moved by 1, 2 and 3 bytes inside its guards: ten outputs, all the
    oracle's bytes."""
    rng = np.random.default_rng(40 + predictor)
    for bw in (4, 64, 65, 257):
        for bh, keep in ((3, bw), (3, 1)):
            nx, ny, _, _ = lc.geometry(bw, bh, keep)
            blocks = lc.random_blocks(rng, nx * ny, bw * bh * 4)
            outs = [run(None, 1, 4, bw, bh, 0, keep, predictor, blocks=blocks)]
            for shift in (1, 2, 3):
                outs.append(run(None, 1, 4, bw, bh, 0, keep, predictor, blocks=blocks, blocks_shift=shift))
                padded = np.concatenate([blocks, lc.random_blocks(rng, nx * ny, shift)], axis=1)
                outs.append(run(None, 1, 4, bw, bh, shift, keep, predictor, blocks=padded))
                outs.append(run(None, 1, 4, bw, bh, 0, keep, predictor, blocks=blocks, image_shift=shift))
            assert len(outs) == 10
            for k, (got, want) in enumerate(outs):
                assert np.array_equal(want, outs[0][1]) and np.array_equal(got, want), (bw, keep, k)


def test_uint16_buffers_at_an_odd_word():
    """uint16 blocks and image at a 2-byte address that is no multiple of 4."""
    rng = np.random.default_rng(5)
    for bw in (3, 64, 257):
        for spp in (1, 2, 3, 4):
            for keep in (1, bw):
                got, want = run(rng, 2, spp, bw, 3, 0, keep, 2, blocks_shift=2, image_shift=2)
                assert np.array_equal(got, want), (bw, spp, keep)


@pytest.mark.parametrize("predictor", [1, 2])
def test_row_groups_cut_by_the_height(predictor):
    """uint8 x 4, one block column, the block as tall as the raster: the wave kernel takes four rows per workgroup, so heights 1, 2, 3,
    5 and 7 leave waves of the last group without a row. The guard begins at the byte behind the last row: a row written past
    ``height`` shows there."""
    rng = np.random.default_rng(60 + predictor)
    for height in (1, 2, 3, 4, 5, 7):
        for bw in (5, 64, 65):
            got, want = run(rng, 1, 4, bw, height, 0, bw, predictor, geom=(1, 1, bw, height))
            assert np.array_equal(got, want), (height, bw)


@pytest.mark.parametrize("item", [1, 2])
def test_refusals_write_nothing(item):
    """Arguments the uint8 and uint16 entries must refuse on the host (the float entry's list is in test_f32_device_gpu.py): ERR_INVALID,
    a message that names the entry point, and not a byte of the image or its guards touched. The buffers are large enough for every
    geometry named here, 65 536 block columns of one pixel included."""
    lib = _lib.load()
    entry = getattr(lib, lc.ENTRY[item])
    sp = _lib.stream_ptr()
    bw, bh, nx, ny, spp, width, height = 16, 8, 2, 2, 2, 30, 13
    cap = bw * bh * spp * item
    d_blocks = torch.zeros((max(9 * cap, 65536 * item) + 16,), dtype=torch.uint8, device="cuda")
    nbytes = max(3 * bw * 3 * bh * spp, 65536) * item
    d_image = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    ok = (d_blocks.data_ptr(), cap, bw, bh, nx, ny, spp, 2, d_image.data_ptr() + GUARD, width, height, sp)
    d_first = torch.full_like(d_image, 0xFF)
    assert entry(*ok[:8], d_first.data_ptr() + GUARD, *ok[9:]) == 0        # the arguments every case below departs from are valid
    torch.cuda.synchronize()
    assert not d_first[GUARD:GUARD + width * height * spp * item].cpu().numpy().any()
    cases = [("null blocks", {0: None}), ("null image", {8: None}), ("spp 0", {6: 0}), ("spp 5", {6: 5}),
             ("predictor 0", {7: 0}), ("predictor 3", {7: 3}), ("predictor 4", {7: 4}),
             ("a block column too many", {4: nx + 1}), ("a block column too few", {4: nx - 1}),
             ("a block row too many", {5: ny + 1}), ("a block row too few", {5: ny - 1}),
             ("block_cap one sample too small", {1: cap - item}),
             ("65 536 block columns", {1: item, 2: 1, 3: 1, 4: 65536, 5: 1, 6: 1, 9: 65536, 10: 1})]
    if item == 2:
        cases += [("odd block_cap", {1: cap + 1}), ("blocks at an odd byte", {0: ok[0] + 1}), ("image at an odd byte", {8: ok[8] + 1})]
    for label, change in cases:
        bad = list(ok)
        for k, v in change.items():
            bad[k] = v
        assert entry(*bad) == _lib.ERR_INVALID, label
        assert lc.ENTRY[item] in lib.td_last_error().decode(), label
    # 65 535 block columns, the most a launch takes, are served
    wide = list(ok)
    for k, v in {1: item, 2: 1, 3: 1, 4: 65535, 5: 1, 6: 1, 9: 65535, 10: 1}.items():
        wide[k] = v
    wide[8] = d_first.data_ptr() + GUARD
    d_first.fill_(0xFF)
    assert entry(*wide) == 0
    torch.cuda.synchronize()
    got = d_first.cpu().numpy()
    assert not got[GUARD:GUARD + 65535 * item].any() and (got[:GUARD] == 0xFF).all() and (got[GUARD + 65535 * item:] == 0xFF).all()
    assert (d_image.cpu().numpy() == 0xFF).all(), "a refused call wrote"
