"""tests/layout_cases.py means what tests/test_layout_kernels_gpu.py takes it for, shown on the CPU: answers worked by hand, the oracle
against the host twins (td_tiff_unpredict, td_tiff_unpredict_float: code this test did not write) at every width and band count, sums
that really wrap, and every faulty variant of DEFECTS changing the expected bytes of a case of the GPU sweep — per kernel it could
live in."""
import numpy as np
import pytest

import layout_cases as lc
from treedetection_amd import _lib


def _one_block(rows, item, bw, spp, predictor):
    """Block rows [bh, bw * spp * item] bytes as ONE block that is the whole raster → [bh, bw, spp]."""
    bh = rows.shape[0]
    return lc.oracle(rows.reshape(1, -1), item, bw, bh, 1, 1, spp, predictor, bw, bh)


def test_known_answers():
    """By hand.
    uint8, predictor 2: 250, 10, 10 → 250, 260 - 256 = 4, 14.
    uint16, predictor 2: 65000, 500, 100 → 65000, 65500, 65600 - 65536 = 64; with two bands the sums skip a sample:
      (1, 2), (65535, 3) → (1, 2), (0, 5).
    float32, predictor 3, 1.0f = 0x3F800000: the planes, most significant first, are 3F | 80 | 00 | 00; differenced with stride 1 over the
      four bytes: 3F, 80 - 3F = 41, 00 - 80 = 80, 00 - 00 = 00.
    Three bands, two pixels (1.0, 2.0, -1.0), (0.5, 1.0, -2.0) = 3F800000 40000000 BF800000, 3F000000 3F800000 C0000000; n = 6:
      plane 0 = 3F 40 BF 3F 3F C0, plane 1 = 80 00 80 00 80 00, planes 2 and 3 = 0. Differences with stride 3 over the 24 bytes:
      3F 40 BF | 3F-3F=00 3F-40=FF C0-BF=01 | 80-3F=41 00-3F=C1 80-C0=C0 | 00-80=80 80-00=80 00-80=80 | 00-00=00 00-80=80 00-00=00 | 0 …"""
    assert _one_block(np.array([[250, 10, 10]], np.uint8), 1, 3, 1, 2).reshape(-1).tolist() == [250, 4, 14]
    row = np.array([[65000, 500, 100]], np.uint16).view(np.uint8)
    assert _one_block(row, 2, 3, 1, 2).reshape(-1).tolist() == [65000, 65500, 64]
    row = np.array([[1, 2, 65535, 3]], np.uint16).view(np.uint8)
    assert _one_block(row, 2, 2, 2, 2).reshape(-1).tolist() == [1, 2, 0, 5]
    one = _one_block(np.array([[0x3F, 0x41, 0x80, 0x00]], np.uint8), 4, 1, 1, 3)
    assert one.dtype == np.uint32 and one.reshape(-1).tolist() == [0x3F800000] and one.view(np.float32).item() == 1.0
    enc = [0x3F, 0x40, 0xBF, 0x00, 0xFF, 0x01, 0x41, 0xC1, 0xC0, 0x80, 0x80, 0x80, 0x00, 0x80, 0x00] + [0] * 9
    pair = _one_block(np.array([enc], np.uint8), 4, 2, 3, 3)
    assert pair.view(np.float32).reshape(-1).tolist() == [1.0, 2.0, -1.0, 0.5, 1.0, -2.0]
    # predictor 1 copies, and only the part of a block inside the raster lands in it: 2 x 2 blocks of 2 x 2 on a 3 x 3 raster
    blocks = np.arange(16, dtype=np.uint8).reshape(4, 4)
    assert lc.oracle(blocks, 1, 2, 2, 2, 2, 1, 1, 3, 3)[:, :, 0].tolist() == [[0, 1, 4], [2, 3, 6], [8, 9, 12]]
    # capacity behind a block is not data
    padded = np.concatenate([blocks, np.full((4, 3), 99, np.uint8)], axis=1)
    assert np.array_equal(lc.oracle(padded, 1, 2, 2, 2, 2, 1, 2, 3, 3), lc.oracle(blocks, 1, 2, 2, 2, 2, 1, 2, 3, 3))


def test_geometry_and_tables():
    assert lc.geometry(64, 3, 1) == (3, 2, 129, 5) and lc.geometry(513, 4, 513) == (2, 2, 1026, 6) and lc.geometry(5, 1, 5) == (3, 2, 15, 2)
    for item in (1, 2, 4):
        cases = list(lc.sweep(item))
        seen = {(spp, bh, pad, keep == 1) for spp, bw, bh, pad, keep in cases}
        assert seen >= {(spp, bh, pad, k1) for spp in (1, 2, 3, 4) for bh in lc.HEIGHTS_BH for pad in lc.PADS[item] for k1 in (False, True)}
        assert {(spp, bw) for spp, bw, *_ in cases} == {(spp, bw) for spp in (1, 2, 3, 4) for bw in lc.WIDTHS}
    # the wave kernel meets a last row group that the height cuts, with an edge block of one pixel; its generic twin (a capacity that is
    # no multiple of 4) does too
    kinds = {(lc.kernel_of(1, spp, 2, bw * bh * spp + pad), bh, keep == 1) for spp, bw, bh, pad, keep in lc.sweep(1) if spp == 4}
    assert kinds >= {("rgbi", 3, True), ("generic", 3, True), ("rgbi", 4, True), ("rgbi", 1, False)}


@pytest.mark.parametrize("item,predictor", [c for c in lc.KERNEL_CASES if c[1] != 1])
def test_the_oracle_equals_the_host_twins_at_every_width(item, predictor):
    lib = _lib.load()
    rng = np.random.default_rng(7 * item + predictor)
    name = "td_tiff_unpredict_float" if predictor == 3 else "td_tiff_unpredict"
    for bw in lc.WIDTHS + (lc.LONG_WIDTH,):
        for spp in (1, 2, 3, 4):
            rows = np.concatenate([lc.random_blocks(rng, 3, bw * spp * item), lc.crafted_rows(item, spp, bw, predictor)])
            twin = rows.copy()
            _lib.check(getattr(lib, name)(twin.ctypes.data, twin.shape[0], bw, spp, item), name)
            want = _one_block(rows, item, bw, spp, predictor)
            assert np.array_equal(want.reshape(-1).view(np.uint8), twin.reshape(-1)), (bw, spp)
            # the crafted rows say what they promise: every pixel equals the first; every step wraps
            const, wrap = want[3], want[4]
            assert const.all() and (const == const[0]).all(), (bw, spp)
            if predictor == 2:
                step = np.arange(1, bw + 1, dtype=np.uint64)[:, None] * np.uint64(np.iinfo(lc.DTYPE[item]).max)
                assert np.array_equal(wrap, (step % np.uint64(1 << 8 * item)).astype(lc.DTYPE[item]).repeat(spp, axis=1)), (bw, spp)
            else:
                sums = lc.fp_byte_sums(rows[4:5], spp)[0]
                assert np.array_equal(sums, (255 * (1 + np.arange(4 * bw * spp) // spp) % 256).astype(np.uint8)), (bw, spp)


@pytest.mark.parametrize("item,predictor", [c for c in lc.KERNEL_CASES if c[1] != 1])
def test_the_random_inputs_of_the_sweep_wrap(item, predictor):
    """A sum that never passed the modulus would let a kernel that widens or clamps go unseen: in every case of the sweep that has a
    left neighbour at all (bw > 1), some sample is smaller than its left neighbour's sum plus its own difference."""
    for (spp, bw, bh, pad, keep), geom, cap, blocks in lc.sweep_inputs(item, predictor):
        data = blocks[:, :bw * bh * spp * item]
        if predictor == 3:
            diff = data.reshape(-1, 4 * bw, spp)            # stride spp over the 4n bytes of a row: a "pixel" is spp bytes
        else:
            diff = data.reshape(-1).view(lc.DTYPE[item]).reshape(-1, bw, spp)
        sums = np.cumsum(diff, axis=1, dtype=diff.dtype)
        unwrapped = sums[:, :-1].astype(np.uint64) + diff[:, 1:]
        assert bw == 1 and predictor == 2 or (sums[:, 1:] < unwrapped).any(), (spp, bw, bh, pad, keep)


def _launch_kernel(item, predictor, case):
    """The kernel a case of the sweep takes; the generic kernel's uint8 four-band instance, which only a capacity or an address that is no
    multiple of 4 reaches, under a name of its own."""
    spp, bw, bh, pad, keep = case
    kind = lc.kernel_of(item, spp, predictor, bw * bh * spp * item + pad)
    return "generic <uint8_t, 4>" if (kind, item, spp) == ("generic", 1, 4) else kind


def test_every_defect_changes_a_case_of_the_sweep():
    """No kernel runs here. For every kernel a defect could live in — (entry, predictor) x {rgbi, generic, plane} as the launcher
    chooses — the first case of the GPU sweep (same seeds, same geometry) whose expected bytes the defect changes is printed; one that
    no case caught would mean the sweep could not tell that kernel from its faulty form. A carry lost between thread runs counts only
    where a run is two pixels or more (bw > 256): below that it is no sum at all, which any case catches."""
    generic = {"generic", "generic <uint8_t, 4>"}
    homes = {"carry_lost_at_64": {"rgbi"}, "carry_lost_at_run": generic, "carry_lost_at_256_bytes": {"plane"},
             "plane_carry_dropped": {"plane"}, "phase_zero_for_three_bands": {"plane"}}
    telling = {"carry_lost_at_run": lambda case: case[1] > 256}
    caught = {}
    for item, predictor in lc.KERNEL_CASES:
        kinds = {"plane"} if predictor == 3 else generic | {"rgbi"} if item == 1 else {"generic"}
        todo = {(name, kind) for name, d in lc.DEFECTS.items() if predictor in d.predictors for kind in kinds if kind in homes.get(name, kinds)}
        for case, (nx, ny, width, height), cap, blocks in lc.sweep_inputs(item, predictor):
            kind = _launch_kernel(item, predictor, case)
            mine = [name for name, k in todo if k == kind and telling.get(name, lambda case: True)(case)]
            if not mine:
                continue
            spp, bw, bh, pad, keep = case
            want = lc.oracle(blocks, item, bw, bh, nx, ny, spp, predictor, width, height)
            for name in mine:
                if not np.array_equal(lc.DEFECTS[name](blocks, item, bw, bh, nx, ny, spp, predictor, width, height), want):
                    todo.discard((name, kind))
                    caught.setdefault(name, []).append((item, predictor, kind, case))
            if not todo:
                break
        assert not todo, f"item {item}, predictor {predictor}: no case of the sweep catches {sorted(todo)}"
    print()
    for name, d in lc.DEFECTS.items():
        assert caught.get(name), f"{name} ({d.what}) is caught by no case"
        for item, predictor, kind, (spp, bw, bh, pad, keep) in caught[name]:
            print(f"{name}: {lc.ENTRY[item]} predictor {predictor}, {kind} kernel: spp {spp}, bw {bw}, bh {bh}, pad {pad}, keep {keep}")
    # the crafted rows catch the lost carries on their own: a constant row turns 0 where the carry is dropped
    for name, item, spp, bw, predictor in (("carry_lost_at_64", 1, 4, 65, 2), ("carry_lost_at_run", 2, 3, 257, 2), ("carry_lost_at_run", 1, 4, 513, 2),
                                          ("carry_lost_at_256_bytes", 4, 1, 257, 3), ("plane_carry_dropped", 4, 2, 65, 3),
                                          ("phase_zero_for_three_bands", 4, 3, 65, 3), ("saturating_add", 4, 4, 65, 2)):
        rows = lc.crafted_rows(item, spp, bw, predictor).reshape(1, -1)
        args = (rows, item, bw, 2, 1, 1, spp, predictor, bw, 2)
        assert not np.array_equal(lc.DEFECTS[name](*args), lc.oracle(*args)), name
