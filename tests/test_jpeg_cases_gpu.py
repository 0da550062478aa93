"""The device JPEG decoder (jpegdecode.hip: jpeg_entropy_kernel, jpeg_entropy_sync_kernel, jpeg_dc_scan_kernel, jpeg_idct_kernel,
jpeg_pixels_kernel / jpeg_pixels4_kernel) on the crafted block sets of tests/jpeg_cases.py, which tests/test_jpeg_cases.py pins on the
CPU: several table sets, sampling modes and coefficient counts in one launch, optimised Huffman tables, steps of 255, frames taller
than their block, rasters of a few pixels, waves that take a second segment of another table set, counts at the wave boundary, and
every 5th bit of three streams flipped — byte for byte against Pillow's libjpeg (the flips: against the host twin, status included),
through all three decoder forms: one lane per segment (td_tiff_jpeg_decode_dev) and one wave per segment (td_tiff_jpeg_decode_long_dev
with long_threshold 0) at subsequences of 8 and 256 bytes. The wave decoder's counts equal the host emulation's (td_jpeg_decode_sync
with 64 lanes), as treedet.h says. Every buffer the kernels write lies between canaries. None of this makes a kernel fault: corrupt
data is data the decoder reports."""
import os
import sys

import numpy as np
import pytest
import torch

from treedetection_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # (pytest's default import mode does this; importlib mode does not)
import jpeg_cases as jc  # noqa: E402

pytestmark = pytest.mark.gpu
SUBSEQS = (8, jc.DEFAULT_SUBSEQ)


def host_stats(case, subseq):
    """What treedet.h says td_tiff_jpeg_decode_long_dev counts over the long segments — {rounds summed over the windows, windows, the
    most rounds one window took, windows of one round} — from the host emulation of every (valid) block's stream with 64 lanes."""
    cache, total = {}, [0, 0, 0, 0]
    for stream in case.blocks:
        if stream not in cache:
            got, st = jc.host_decode_sync(stream, subseq, 64)
            assert not isinstance(got, int)
            cache[stream] = st
        r, w, m, s = cache[stream]
        total = [total[0] + r, total[1] + w, max(total[2], m), total[3] + s]
    return total


def all_forms(case, expect_status=None, stats=True):
    """The case through the three decoder forms; the wave forms' stats against the host twin's unless the case holds corrupt blocks."""
    pl = jc.plan(case)
    jc.check(case, jc.decode_on_device(case, pl=pl), expect_status)
    for subseq in SUBSEQS:
        res = jc.decode_on_device(case, long_threshold=0, subseq_bytes=subseq, pl=pl)
        assert res.long_segments == len(pl.segs)
        jc.check(case, res, expect_status)
        if stats:
            assert res.stats == host_stats(case, subseq), (case.name, subseq, res.stats)


@pytest.mark.parametrize("variant", list(jc.MIXED))
def test_mixed(variant):
    all_forms(jc.mixed(variant))


@pytest.mark.parametrize("mode", jc.TINY_MODES)
@pytest.mark.parametrize("size", jc.TINY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny(size, mode):
    all_forms(jc.tiny(size, mode))


def test_restage():
    """More long segments than the wave launch has waves, drawn from P table sets: some wave takes a second segment of another set and
    must restage its LDS copy. The copy serves the Huffman tables and the range check, so a stale one shows where the Huffman tables
    change — about two of three changes of set, those that touch an optimize=True stream: a false status or other pixels (the second
    control of test_jpeg_cases.py). Every form also reads `sets` per block for the DC scan and the IDCT: the wrong one there decodes
    without error to other pixels (the first control)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case, _ = jc.restage(cus)
    pl = jc.plan(case)
    nseg, waves = len(pl.segs), jc.restage_waves(len(pl.segs), cus)
    print(f"\nrestage: {cus} CUs, {len(case.blocks)} blocks, {len(pl.sets)} table sets, {nseg} long segments for {waves} waves "
          f"({nseg - waves} second tickets at the least)")
    assert len(pl.sets) == jc.POOL_SIZE and nseg == len(case.blocks) >= 4 * cus + 256 and nseg > waves
    jc.check(case, jc.decode_on_device(case, pl=pl))
    for subseq in SUBSEQS:
        res = jc.decode_on_device(case, long_threshold=0, subseq_bytes=subseq, runs=2, pl=pl)
        assert res.long_segments == nseg
        jc.check(case, res)
        (image, status, stats), = res.earlier
        assert np.array_equal(image, res.image) and np.array_equal(status, res.status) and stats == res.stats
        assert res.stats == host_stats(case, subseq), (subseq, res.stats)


@pytest.mark.parametrize("name", jc.WAVE_DC)
def test_wave_counts_dc(name):
    """63 / 64 / 65 blocks of one component in one segment, 64 chroma and 256 luma blocks: the DC scan's carry across 64-block steps."""
    all_forms(jc.wave_dc(name))


@pytest.mark.parametrize("name,target", jc.WAVE_CASES)
def test_wave_counts_subsequences(name, target):
    """One segment cut into exactly `target` subsequences: a window of 63, 64 and 65 (a second window of one lane), two full windows, two
    and one."""
    case = jc.wave_stream(name)
    pl = jc.plan(case)
    subseq = jc.wave_subseq(int(pl.segs[0, 1]), target)
    assert jc.subsequences(int(pl.segs[0, 1]), subseq) == target
    res = jc.decode_on_device(case, long_threshold=0, subseq_bytes=subseq, pl=pl)
    jc.check(case, res)
    want = host_stats(case, subseq)
    assert want[1] == -(-target // 64)
    assert res.stats == want, (target, subseq, res.stats, want)


@pytest.mark.parametrize("name", jc.FLIP_STREAMS)
def test_flips(name):
    """Every flipped stream the plan accepts, in one launch per decoder form, between two copies of the valid stream: the host twin's
    status on every block and its bytes on every block it decodes."""
    f = jc.flips(name)
    print(f"\nflips {name}: {len(f.case.blocks) - 2} of {f.total} flipped streams launched, {int(f.expect_status.sum())} expected corrupt")
    all_forms(f.case, f.expect_status, stats=False)


def _refused(fn, name, args, changes, message):
    lib = _lib.load()
    bad = list(args)
    for k, v in changes.items():
        bad[k] = v
    assert fn(*bad) == _lib.ERR_INVALID, (name, changes)
    err = lib.td_last_error().decode()
    assert name in err and message in err, (changes, err)


@pytest.mark.parametrize("variant", ["rgb", "four"])
def test_the_entry_points_refuse_before_any_launch(variant):
    """Every refusal returns TD_ERR_INVALID with a message and leaves coef, planes, status, stats and image untouched (nothing ran)."""
    lib = _lib.load()
    case = jc.mixed(variant)
    d = jc.Device(case)
    nb = len(case.blocks)
    dev, name = d.args_dev(), "td_tiff_jpeg_decode_dev"
    for k in (0, 1, 3, 5, 6, 7, 9, 10):
        _refused(lib.td_tiff_jpeg_decode_dev, name, dev, {k: None}, "null pointer")
    _refused(lib.td_tiff_jpeg_decode_dev, name, dev, {6: dev[6] + 2}, "16-byte aligned")
    _refused(lib.td_tiff_jpeg_decode_dev, name, dev, {4: nb - 1}, "segments")
    _refused(lib.td_tiff_jpeg_decode_dev, name, dev, {8: dev[8] + 1}, "coefficients")
    for changes in ({11: 145}, {11: 96}, {12: 97}, {12: 64}, {16: 2}, {16: 4}, {13: 2}, {14: 0}):
        _refused(lib.td_tiff_jpeg_decode_dev, name, dev, changes, "do not tile")
    lng, name = d.args_long(0), "td_tiff_jpeg_decode_long_dev"
    assert lng[3] is None and lng[4] == 0 and lng[6] == len(d.plan.segs)
    for k in (0, 1, 5, 8, 9, 10, 12, 13, 14):
        _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {k: None}, "null pointer")
    _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {3: None, 4: 5}, "null pointer")
    _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {9: lng[9] + 2}, "16-byte aligned")
    _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {13: lng[13] + 4}, "8-byte aligned")
    _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {6: nb - 1}, "segments")
    for s in (3, (1 << 20) + 1, 0, -8):
        _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {7: s}, "subsequences of")
    for changes in ({15: 145}, {15: 96}, {16: 97}, {16: 64}, {20: 2}, {20: 4}, {17: 2}, {18: 0}):
        _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, changes, "do not tile")
    if case.bands == 4:
        for off in (1, 2, 3):
            _refused(lib.td_tiff_jpeg_decode_dev, "td_tiff_jpeg_decode_dev", dev, {10: dev[10] + off}, "4-byte aligned")
            _refused(lib.td_tiff_jpeg_decode_long_dev, name, lng, {14: lng[14] + off}, "4-byte aligned")
    assert d.untouched()
    # ... and the same arguments unchanged decode the case
    _lib.check(lib.td_tiff_jpeg_decode_dev(*dev), "td_tiff_jpeg_decode_dev")
    img, status, _, alive = d.fetch(False)
    jc.check(case, jc.Result(img, status, None, alive))
