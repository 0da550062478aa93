"""Long entropy-coded segments decoded by many lanes (self-synchronising Huffman decoding, jpeg_core.h): the window procedure that
one wave runs on the GPU (jpegdecode.hip: jpeg_entropy_sync_kernel), run here by one host thread over emulated lanes
(td_jpeg_decode_sync) — against Pillow's libjpeg byte for byte, and against the sequential decoder (td_jpeg_decode) on corrupt data:
the same pixels or the same error."""
import glob
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, device_decode_long_jpeg_setting, write_geotiff

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
SUBSEQ = (8, 32, 128, 512)
LANES = (1, 2, 64)
JPEG4 = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "jpeg4", "*.jpg")))


def _call(name, stream: bytes, *extra):
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8)
    out = np.zeros(1 << 21, dtype=np.uint8)
    shape = np.zeros(3, dtype=np.int32)
    n = getattr(lib, name)(src.ctypes.data, src.size, out.ctypes.data, out.size, shape.ctypes.data, *extra)
    if n < 0:
        return n
    h, w, c = (int(v) for v in shape)
    assert n == h * w * c
    arr = out[:n].reshape(h, w, c)
    return arr[:, :, 0] if c == 1 else arr


def decode(stream: bytes):
    return _call("td_jpeg_decode", stream)


def decode_sync(stream: bytes, subseq: int, lanes: int, stats=None):
    st = np.zeros(4, dtype=np.int64)
    got = _call("td_jpeg_decode_sync", stream, subseq, lanes, st.ctypes.data)
    if stats is not None:
        stats[:] = st
    return got


def encode(img: np.ndarray, mode: str, **kw) -> bytes:
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        buf = io.BytesIO()
        if mode == "L":
            Image.fromarray(img[:, :, 0]).save(buf, "JPEG", **kw)
        else:
            Image.fromarray(img).save(buf, "JPEG", subsampling=SUBSAMPLING[mode], **kw)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def pillow(stream: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(stream)) as im:
        return np.asarray(im)


def image(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def assert_sync_equals(stream: bytes, ref: np.ndarray, subseqs=SUBSEQ, lanes=LANES):
    for s in subseqs:
        for l in lanes:
            got = decode_sync(stream, s, l)
            assert not isinstance(got, int), f"td_jpeg_decode_sync({s}, {l}) returned {got}: {_lib.load().td_last_error()}"
            assert got.shape == ref.shape and np.array_equal(got, ref), (s, l, got.shape, ref.shape, int((got != ref).sum()))


@pytest.mark.parametrize("mode", ["L", "444", "422", "420"])
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_matches_pillow(mode, quality, kind):
    """Every subsequence size and lane count, on a stream of less than one subsequence (1x1), of a few (17x33) and of many windows."""
    for size in ((1, 1), (17, 33), (517, 683)):
        stream = encode(image(*size, kind), mode, quality=quality)
        assert_sync_equals(stream, pillow(stream))


@pytest.mark.parametrize("path", JPEG4, ids=[os.path.basename(p) for p in JPEG4])
def test_four_component_streams_match_their_stored_bytes(path):
    """The committed four-component streams (mode 4: four blocks per MCU, four DC predictors) against the bytes libjpeg stores for them."""
    stream = open(path, "rb").read()
    want = np.fromfile(path[:-4] + ".raw", dtype=np.uint8)
    ref = decode(stream)
    assert ref.shape[2] == 4 and np.array_equal(ref.ravel(), want)
    assert_sync_equals(stream, ref)


def test_four_component_fixtures_are_there():
    assert len(JPEG4) >= 2


@pytest.mark.parametrize("mode", ["L", "444", "422", "420"])
@pytest.mark.parametrize("opts", [{"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1},
                                  {"restart_marker_blocks": 5, "optimize": True}])
def test_optimized_tables_and_restart_intervals(mode, opts):
    for kind in ("noise", "smooth"):
        stream = encode(image(71, 133, kind, seed=3), mode, quality=90, **opts)
        assert_sync_equals(stream, pillow(stream))


def test_short_subsequences_need_rounds_and_sometimes_none():
    """At 8 bytes a block spans many subsequences and symbols straddle the boundaries: most guesses are wrong and the true state has
    to travel (windows of more than two rounds), while a window whose guesses all hold — at the least a segment's last window of one
    lane — takes exactly one. Both in one stream; then each kind by construction."""
    stats = np.zeros(4, dtype=np.int64)
    stream = encode(image(96, 128, "smooth", seed=1), "420", quality=90)
    got = decode_sync(stream, 8, 64, stats)
    assert np.array_equal(got, pillow(stream))
    rounds, windows, most, single = (int(v) for v in stats)
    assert windows == (len(stream) - _entropy_start(stream) - 2 + 8 * 64 - 1) // (8 * 64) and rounds >= windows
    assert 2 < most <= 64 and single >= 1, stats
    # a restart marker after every block of a flat image: every segment is one window of one or two subsequences, guessed right or not at all
    flat = encode(np.full((16, 64, 3), 90, dtype=np.uint8), "L", quality=90, restart_marker_blocks=1)
    got = decode_sync(flat, 8, 64, stats)
    assert np.array_equal(got, pillow(flat))
    assert int(stats[1]) == 16 and int(stats[3]) >= 1, stats
    noise = encode(image(96, 128, "noise", seed=1), "420", quality=90)
    got = decode_sync(noise, 8, 64, stats)
    assert np.array_equal(got, pillow(noise))
    assert int(stats[2]) > 2 and int(stats[0]) > 2 * int(stats[1]), stats
    # one lane per window: lane 0 enters with the true state, every window takes exactly one round
    decode_sync(noise, 8, 1, stats)
    assert int(stats[0]) == int(stats[1]) == int(stats[3]) and int(stats[2]) == 1, stats


def _entropy_start(stream: bytes) -> int:
    sos = stream.index(b"\xff\xda")
    return sos + 2 + ((stream[sos + 2] << 8) | stream[sos + 3])


def test_a_subsequence_boundary_between_ff_and_its_stuffed_zero():
    """Noise at quality 100 is full of FF 00 pairs; seed 2 puts a boundary of every tested subsequence size between an FF and its 00
    (verified on the bytes: the lane that starts there must skip the 00, and the lane before it must end past it)."""
    stream = encode(image(64, 96, "noise", seed=2), "444", quality=100)
    e0 = _entropy_start(stream)
    data = np.frombuffer(stream, dtype=np.uint8)[e0:-2]
    at = np.nonzero((data[:-1] == 0xFF) & (data[1:] == 0))[0] + 1          # offsets of the stuffed zeros in the segment
    assert at.size > 50
    for s in (8, 32, 128):
        assert (at % s == 0).any(), f"no FF | 00 boundary at subsequences of {s} bytes: choose another seed"
    assert_sync_equals(stream, pillow(stream), subseqs=(8, 32, 128), lanes=(2, 3, 64))


def test_bit_flips_and_prefixes_give_what_the_sequential_decoder_gives():
    """300 seeded bit flips in the entropy-coded data and every 97th prefix of a 4:2:0 stream: the same error code or the same pixels."""
    rng = np.random.default_rng(23)
    stream = encode(image(96, 128, "smooth", seed=4), "420", quality=90)
    start = _entropy_start(stream)
    errors = decoded = 0
    for i in range(300):
        bad = bytearray(stream)
        pos = int(rng.integers(start, len(stream) - 2))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        want = decode(bytes(bad))
        got = decode_sync(bytes(bad), (8, 32, 128)[i % 3], (2, 64, 3)[(i // 3) % 3])
        if isinstance(want, int):
            assert isinstance(got, int) and got == want == _lib.ERR_INVALID, (pos, got, want)
            errors += 1
        else:
            assert not isinstance(got, int) and np.array_equal(got, want), pos
            decoded += 1
    assert errors > 0 and decoded > 0, (errors, decoded)
    for k, cut in enumerate(range(0, len(stream), 97)):
        want = decode(stream[:cut])
        got = decode_sync(stream[:cut], (8, 32, 128)[k % 3], 64)
        assert isinstance(want, int) and isinstance(got, int) and got == want, (cut, got, want)


def test_arguments_are_checked():
    stream = encode(image(16, 16, "smooth"), "420", quality=90)
    for s, l in ((3, 64), (0, 64), ((1 << 20) + 1, 64), (32, 0), (32, 65)):
        assert decode_sync(stream, s, l) == _lib.ERR_INVALID
        assert b"td_jpeg_decode_sync" in _lib.load().td_last_error()


def test_rasters_with_long_segments_are_decodable_when_asked(tmp_path):
    """The raster of test_rasters_with_segments_beyond_the_lane_limit_stay_on_the_host: still refused by default."""
    data = image(1024, 1024, "noise").transpose(2, 0, 1)
    one = str(tmp_path / "one.tif")
    write_geotiff(one, data, (1, 0, 0, 0, -1, 1024), compression="jpeg", rows_per_strip=1024)
    g = GeoTiff(one)
    g._setup_blocks()
    assert g._counts[0] > GeoTiff.JPEG_DEVICE_MAX_SEGMENT
    assert g.device_decodable(long_segments=True) is True
    assert g.device_decodable() is False and g.device_decodable(long_segments=False) is False
    g.close()


def test_both_stages_read_the_long_jpeg_key_the_same_way(monkeypatch):
    import treedetection_amd as TD
    from treedetection_amd import postprocessing as P
    assert device_decode_long_jpeg_setting() is False and device_decode_long_jpeg_setting(None) is False
    assert device_decode_long_jpeg_setting(True) is True and device_decode_long_jpeg_setting("true") is True
    assert device_decode_long_jpeg_setting(False) is False and device_decode_long_jpeg_setting("false") is False
    for bad in ("auto", "all", 1, 0, "yes", 2.0):
        with pytest.raises(ValueError, match="device_decode_long_jpeg"):
            device_decode_long_jpeg_setting(bad)
        with pytest.raises(ValueError, match="device_decode_long_jpeg"):
            P._long_jpeg_on({"device_decode_long_jpeg": bad})
        with pytest.raises(ValueError, match="device_decode_long_jpeg"):
            TD.Predictor(None, device_decode_long_jpeg=bad)
    assert P._long_jpeg_on({}) is False and P._long_jpeg_on({"device_decode_long_jpeg": "true"}) is True
    assert P._long_jpeg_on({"device_decode_long_jpeg": False}) is False


GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "jpegsync", "*.jpg")))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_committed_streams_of_the_sanitizer_program_match_pillow(path):
    """tests/golden/jpegsync (make_jpegsync_fixture.py): what checks/jpegsync_check.cpp compares the two decoders on."""
    stream = open(path, "rb").read()
    assert_sync_equals(stream, pillow(stream), subseqs=(8, 32, 128), lanes=(1, 3, 64))


def test_the_sanitizer_program_has_its_streams():
    assert len(GOLDEN) == 5
