"""The crafted block sets of tests/jpeg_cases.py mean what they claim, on the CPU: every block decodes on the host twin (td_jpeg_decode)
as Pillow's libjpeg decodes it, td_tiff_jpeg_plan accepts every case, the properties each family exists for are there (several table
sets, modes and coefficient counts in one plan; exactly P sets without long runs of one; the subsequence counts at the wave boundary;
the bit flips' shares of refusals, errors and decodes), and the checker the GPU tests use rejects what a wrong kernel would produce."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # (pytest's default import mode does this; importlib mode does not)
import jpeg_cases as jc  # noqa: E402

MI355X_CUS = 256


def _blocks_equal_pillow(case):
    for b, stream in enumerate(dict.fromkeys(case.blocks)):
        got = jc.host_decode(stream)
        assert not isinstance(got, int), (case.name, b, got)
        ref = jc.pillow(stream)
        assert got.shape == ref.shape and np.array_equal(got, ref), (case.name, b, int((got != ref).sum()))


@pytest.mark.parametrize("variant", list(jc.MIXED))
def test_mixed(variant):
    case = jc.mixed(variant)
    _blocks_equal_pillow(case)
    pl = jc.plan(case)
    info = pl.info
    assert len(pl.sets) >= 6 and info[8, 1] == info[0, 1]                     # the repeat shares block 0's set
    per_block = np.diff(np.append(info[:, 6], pl.ncoef))
    assert len(set(per_block.tolist())) >= 2
    tall = np.nonzero(info[:, 5] > case.bh)[0]                                # a frame taller than the grid's blocks, in a block that
    assert tall.tolist() == [4] and info[4, 5] == 48 and case.rect(4)[2:] == (32, 48)    # keeps all its 32 rows: 16 rows are dropped
    assert (info[:, 7] == 1).any() and (info[:, 7] > 1).any()
    assert set(info[:, 2].tolist()) == {"rgb": {1, 2, 3}, "grey": {0}, "four": {4}}[variant]
    assert (case.width, case.height) == (131, 85) and case.rect(8)[2:] == (21, 35)
    if variant == "rgb":
        assert len(pl.segs) > len(case.blocks)


@pytest.mark.parametrize("mode", jc.TINY_MODES)
@pytest.mark.parametrize("size", jc.TINY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny(size, mode):
    case = jc.tiny(size, mode)
    _blocks_equal_pillow(case)
    pl = jc.plan(case)
    assert pl.info[0, 2] == jc.MODE_OF[mode] and (pl.info[0, 5], pl.info[0, 4]) == size


def test_restage():
    case, draw = jc.restage(MI355X_CUS)
    _blocks_equal_pillow(case)
    pl = jc.plan(case)
    n = len(case.blocks)
    assert n == 1280 and n % case.across == 0 and n >= 4 * MI355X_CUS + 256
    assert len(pl.sets) == jc.POOL_SIZE and len(pl.segs) == n and (pl.info[:, 2] == 3).all()
    assert n > jc.restage_waves(n, MI355X_CUS)                                 # more segments than waves: second tickets are taken
    # the plan's set of a block is its pool stream's, and no set runs on for more than 8 blocks in segment order
    first = {int(i): int(pl.info[np.nonzero(draw == i)[0][0], 1]) for i in range(jc.POOL_SIZE)}
    assert len(set(first.values())) == jc.POOL_SIZE and all(int(pl.info[b, 1]) == first[int(draw[b])] for b in range(n))
    sets = pl.info[pl.segs[:, 2], 1]
    cuts = np.nonzero(np.diff(sets) != 0)[0]
    runs = np.diff(np.concatenate([[-1], cuts, [n - 1]]))
    assert runs.sum() == n and runs.max() <= 8, int(runs.max())
    # a missed restage of the wave kernel shows where the Huffman tables change: a change of set that touches an optimize=True stream
    # (the control below). Of a uniform draw's changes that is 1 - (6/10 * 5/10) / (9/10) = 2/3; a wave's second segment is some later
    # one, not the next, but drawn alike.
    k = len(jc.RESTAGE_STANDARD)
    by_seg = draw[pl.segs[:, 2]]
    change = by_seg[1:] != by_seg[:-1]
    seen = change & ((by_seg[1:] >= k) | (by_seg[:-1] >= k))
    assert 0.6 * change.sum() <= seen.sum(), (int(seen.sum()), int(change.sum()))
    assert (case.width, case.height) == (case.across * 16 - 3, n // case.across * 16 - 5)


def test_restage_control_a_stale_table_set_decodes_without_error_to_other_pixels():
    """A block decoded with another table set of the pool is wrong and nothing reports it: its stream with another standard-Huffman
    pool stream's quantisation tables decodes WITHOUT error and to OTHER pixels, so only the image check sees a kernel that indexes
    `sets` by the wrong block (jpeg_entropy_kernel, jpeg_dc_scan_kernel's q0, jpeg_idct_kernel's sets[bi[1]].q[c]).

    What this does NOT show is a missed restage in jpeg_entropy_sync_kernel between two of these six streams. That kernel's LDS copy
    serves the Huffman tables and the range check jpeg_coef_ok alone; the coefficients it stores are not dequantised, and the DC scan
    and the IDCT read their tables from global memory. A stale copy of equal Huffman tables stores the same coefficients, and because
    every pair here passes the range check (no error, asserted below), it raises no status either: the pixels come out right. The GPU
    restage test sees a missed restage through the four optimize=True streams, whose Huffman tables differ from the standard ones and
    from each other — test_restage counts the transitions that touch one."""
    pool = jc.restage_pool()
    k = len(jc.RESTAGE_STANDARD)
    for i in range(k):
        ref = jc.pillow(pool[i])
        for j in range(k):
            if i == j:
                continue
            got = jc.host_decode(jc.splice_dqt(pool[i], pool[j]))
            assert not isinstance(got, int), (i, j, got)
            assert got.shape == ref.shape and not np.array_equal(got, ref), (i, j)


def test_restage_control_stale_huffman_tables_give_an_error_or_other_pixels():
    """What a missed restage in jpeg_entropy_sync_kernel does where it can be seen. The six standard streams share their Huffman
    tables; the four optimize=True streams have tables of their own, pairwise different. A pool stream decoded with the Huffman tables
    of a stream whose tables differ is rejected or decodes to other coefficients, hence other pixels: on the device a false status or
    wrong bytes, and check() fails on either. (The host's range check runs with the block's own quantisation tables and a stale LDS set
    brings its own; that changes which of the two outcomes it is, not that the stored coefficients already differ.)"""
    pool = jc.restage_pool()
    k = len(jc.RESTAGE_STANDARD)
    dht = [jc.dht_bytes(s) for s in pool]
    assert len(set(dht[:k])) == 1 and len(set(dht)) == 1 + len(jc.RESTAGE_OPTIMIZED)
    for i, stream in enumerate(pool):
        ref = jc.pillow(stream)
        assert np.array_equal(jc.host_decode(jc.splice_dht(stream, stream)), ref)          # the rebuilt header is a valid one
        for j, donor in enumerate(pool):
            if dht[i] == dht[j]:
                continue
            got = jc.host_decode(jc.splice_dht(stream, donor))
            assert isinstance(got, int) or (got.shape == ref.shape and not np.array_equal(got, ref)), (i, j)


@pytest.mark.parametrize("name", jc.WAVE_DC)
def test_wave_counts_dc(name):
    case = jc.wave_dc(name)
    _blocks_equal_pillow(case)
    pl = jc.plan(case)
    assert len(pl.segs) == 1 and pl.info[0, 7] == 0
    if name == "420-128x128":
        assert pl.ncoef == (256 + 64 + 64) * 64 and pl.info[0, 2] == 3
    else:
        assert pl.ncoef == int(name.split("-")[1]) * 64 and pl.info[0, 2] == 0


@pytest.mark.parametrize("name", list(jc.WAVE_STREAMS))
def test_wave_counts_subsequences(name):
    case = jc.wave_stream(name)
    _blocks_equal_pillow(case)
    pl = jc.plan(case)
    assert len(pl.segs) == 1
    n = int(pl.segs[0, 1])
    e0, e1 = jc.entropy_span(case.blocks[0])
    assert e1 - e0 <= n <= e1 - e0 + 2
    for target in jc.WAVE_STREAMS[name][3]:
        s = jc.wave_subseq(n, target)
        assert 4 <= s <= 1 << 20 and jc.subsequences(n, s) == target
        got, stats = jc.host_decode_sync(case.blocks[0], s)
        assert np.array_equal(got, case.refs[0])
        assert stats[1] == -(-target // 64), (target, s, stats)               # windows of 64 subsequences
    assert set(jc.WAVE_TARGETS) - set(jc.WAVE_STREAMS[name][3]) <= {128}
    assert jc.WAVE_STREAMS["128x96"][3] == jc.WAVE_TARGETS


@pytest.mark.parametrize("name", jc.FLIP_STREAMS)
def test_flips(name):
    f = jc.flips(name)
    refused, errors = int(f.refused.sum()), f.host_errors
    decodes = f.total - errors
    share = lambda k: 100.0 * k / f.total
    print(f"\nflips {name}: {f.total} cases, {share(refused):.1f} % plan refusals, {share(errors):.1f} % host errors, "
          f"{share(decodes):.1f} % host decodes")
    e0, e1 = jc.entropy_span(jc.flip_stream(name))
    assert f.total == -(-8 * (e1 - e0) // jc.FLIP_STRIDE) == len(f.outcomes) == len(f.refused)
    assert refused <= 0.05 * f.total
    assert decodes >= 0.10 * f.total and errors >= 0.10 * f.total
    assert all(isinstance(o, int) and o < 0 for o, r in zip(f.outcomes, f.refused) if r)     # every plan refusal is a host error too
    # only the launch is restricted to the accepted streams: the original, they in order, the original
    accepted = [k for k in range(f.total) if not f.refused[k]]
    assert f.case.blocks == [jc.flip_stream(name)] + [f.streams[k] for k in accepted] + [jc.flip_stream(name)]
    assert f.expect_status.tolist() == [0] + [int(isinstance(f.outcomes[k], int)) for k in accepted] + [0]
    assert all((f.case.refs[b] is None) if isinstance(f.outcomes[k], int) else np.array_equal(f.case.refs[b], f.outcomes[k])
               for b, k in enumerate(accepted, start=1))
    assert jc.plan(f.case).unsupported == 0
    # the emulation of the wave decoder has the sequential decoder's outcome on EVERY flipped stream, the refused ones (forged or
    # broken markers, where a cut into subsequences would depart first) included
    for k, (stream, want) in enumerate(zip(f.streams, f.outcomes)):
        for subseq in (8, 256):
            got, _ = jc.host_decode_sync(stream, subseq, 64)
            if isinstance(want, int):
                assert isinstance(got, int) and got < 0, (k, subseq, bool(f.refused[k]))
            else:
                assert not isinstance(got, int) and np.array_equal(got, want), (k, subseq, bool(f.refused[k]))


def _right(case, status=None):
    nb = len(case.blocks)
    return jc.Result(case.expected.copy(), np.zeros(nb, np.int32) if status is None else status.copy(), None, True)


def test_the_checker_rejects_what_a_wrong_kernel_would_give():
    case = jc.mixed("rgb")
    jc.check(case, _right(case))
    for y, x, c in ((40, 60, 1), (0, 0, 0), (84, 130, 2), (31, 95, 0), (20, 130, 1), (84, 10, 0), (32, 48, 2)):
        r = _right(case)                       # inside a block, the corners, the last kept column / row beside the cropped margin
        r.image[y, x, c] ^= 1
        with pytest.raises(AssertionError, match="differs in 1 bytes"):
            jc.check(case, r)
    r = _right(case)
    r.status[4] = 1
    with pytest.raises(AssertionError, match="status of block 4"):
        jc.check(case, r)
    expect = np.zeros(9, np.int32)
    expect[4] = 1
    with pytest.raises(AssertionError, match="status of block 4"):
        jc.check(case, _right(case), expect_status=expect)
    r = _right(case, expect)
    r.image[40, 60] ^= 1                                                        # block 4: expected corrupt, its pixels are not compared
    jc.check(case, r, expect_status=expect)
    r.image[0, 0, 0] ^= 1
    with pytest.raises(AssertionError, match="block 0 "):
        jc.check(case, r, expect_status=expect)
    r = _right(case)
    r.canaries = False
    with pytest.raises(AssertionError, match="canary"):
        jc.check(case, r)
    shifted = copy.copy(case)
    shifted.expected = np.roll(case.expected, 1, axis=1)
    with pytest.raises(AssertionError, match="differs"):
        jc.check(shifted, _right(case))
