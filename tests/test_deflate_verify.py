"""td_tiff_inflate_verified — the DEFLATE decoder the GPU runs (csrc/inflate_core.h, one lane on the host) with zlib's header and
code-set rules and the Adler-32 trailer check — accepts exactly the streams zlib accepts, and gives zlib's bytes for them."""
import numpy as np

from treedetection_amd import _lib

from deflate_cases import flipped, flips, valid_streams, zlib_outcome


def _run(fn, s, out, cap):
    src = np.frombuffer(s, dtype=np.uint8)
    return int(fn(src.ctypes.data, len(s), out.ctypes.data, cap))


def _disagreements(fn, cases, out, cap):
    """Every case against zlib's outcome → (cases that differ, streams accepted although zlib refuses them)."""
    wrong, lenient = [], 0
    for tag, s in cases:
        d = zlib_outcome(s)
        n = _run(fn, s, out, cap)
        if d is None:
            if n >= 0:
                lenient += 1
                wrong.append((tag, "zlib refuses", n))
        elif len(d) > cap:
            if n != _lib.ERR_CAPACITY:
                wrong.append((tag, "capacity", n))
        elif n != len(d) or out[:n].tobytes() != d:
            wrong.append((tag, len(d), n))
    return wrong, lenient


def test_verified_inflate_agrees_with_zlib_on_every_stream_and_every_flipped_bit():
    lib = _lib.load()
    streams, raws = valid_streams()
    cap = max(len(r) for r in raws) + 64
    out = np.zeros(cap + 16, dtype=np.uint8)
    muts = flips(streams)
    assert len(muts) >= 2000
    for k, s in enumerate(streams):                                     # every header and trailer bit of every stream is among them
        mine = {b for kk, b in muts if kk == k}
        assert set(range(16)) <= mine and set(range(8 * (len(s) - 4), 8 * len(s))) <= mine
    assert sum(1 for k, b in muts if 19 <= b < 24 and (streams[k][2] >> 1) & 3 == 0) >= 5 * 7      # padding in front of a stored LEN
    cases = [((k, None), s) for k, s in enumerate(streams)] + [((k, b), flipped(streams[k], b)) for k, b in muts]
    # zlib accepts some of the flips (padding bits): the rule is not "every flip fails"
    assert any(zlib_outcome(s) is not None for (k, b), s in cases if b is not None)
    # without the check: the decoder that stops at the last end-of-block symbol accepts streams zlib refuses (the trailer flips)
    wrong_plain, lenient_plain = _disagreements(lib.td_tiff_inflate, cases, out, cap)
    assert lenient_plain >= 32, lenient_plain
    wrong, lenient = _disagreements(lib.td_tiff_inflate_verified, cases, out, cap)
    assert not wrong, (len(wrong), wrong[:10])
    assert lenient == 0


def test_capacity_and_truncation_follow_zlib():
    """A stream that zlib accepts but that holds more than the caller's capacity → TD_ERR_CAPACITY; a stream cut anywhere inside its
    trailer, or before it, is incomplete for zlib and refused here; bytes behind the trailer (padding in a strip's byte count) are ignored
    by both."""
    lib = _lib.load()
    streams, raws = valid_streams()
    out = np.zeros(max(len(r) for r in raws) + 80, dtype=np.uint8)
    for s, raw in zip(streams, raws):
        if len(raw) > 100:
            assert _run(lib.td_tiff_inflate_verified, s, out, 100) == _lib.ERR_CAPACITY
        assert _run(lib.td_tiff_inflate_verified, s, out, len(raw)) == len(raw)
        for cut in (1, 2, 3, 4, 5):
            assert zlib_outcome(s[:-cut]) is None
            assert _run(lib.td_tiff_inflate_verified, s[:-cut], out, len(raw)) == _lib.ERR_INVALID, cut
        for pad in (b"\0", b"\xff" * 7):
            assert zlib_outcome(s + pad) == raw
            assert _run(lib.td_tiff_inflate_verified, s + pad, out, len(raw)) == len(raw)
            assert out[:len(raw)].tobytes() == raw
