"""Zstandard on the host (zstd_core.h on one lane: td_tiff_zstd_decode) and ZSTD GeoTIFFs through the block reader. libzstd — the two
builds this machine may have, through ctypes — is the judge where it loads; the committed streams of tests/golden/zstd carry their
own hashes. The same core runs on the GPU: tests/test_zstd_decode_gpu.py."""
import os

import numpy as np
import pytest

import zstd_cases as zc
from treedetection_amd import _lib
from treedetection_amd import geotiff as gt
from treedetection_amd.geotiff import GeoTiff, write_geotiff

MANIFEST = zc.manifest()
STREAMS = {e["name"]: e for e in MANIFEST["streams"]}
TRANSFORM = (0.2, 0, 500000.0, 0, -0.2, 5600000.0)
needs_libzstd = pytest.mark.skipif(not zc.libzstd_builds(), reason="libzstd does not load")


@pytest.fixture(scope="module")
def inputs():
    return zc.inputs()


def test_committed_streams_reproduce_their_hashes():
    for e in MANIFEST["streams"]:
        n, out = zc.decode(zc.load_stream(e), e["length"])
        assert n == e["length"] and zc.sha(out) == e["sha256"], e["name"]
        if "payload_hex" in e:
            assert out.hex() == e["payload_hex"], e["name"]


def test_committed_streams_match_their_inputs(inputs):
    """The generator's inputs are still what the streams were made from (so the fresh-compression tests cover the same data)."""
    for e in MANIFEST["streams"]:
        assert zc.sha(inputs[e["input"]]) == e["sha256"], e["name"]


def test_fixture_size_limits():
    sizes = {f: os.path.getsize(os.path.join(zc.GOLDEN, f)) for f in os.listdir(zc.GOLDEN)}
    assert max(sizes.values()) <= 560 << 10 and sum(sizes.values()) < 1536 << 10
    assert all(v < 100 << 10 for f, v in sizes.items() if f.endswith(".tif"))


def test_committed_streams_reach_every_mode():
    """A later edit cannot thin the coverage: no mode of the list may be missing from the committed streams."""
    total = {}
    for e in MANIFEST["streams"]:
        n, st = zc.stats(zc.load_stream(e))
        assert n == e["length"], e["name"]
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    missing = [m for m in zc.REQUIRED_MODES if not total.get(m)]
    assert not missing, missing
    # the hand-built frames add what libzstd did not emit here
    hand = {}
    for name, (f, exp, _) in zc.hand_frames().items():
        if exp is not None:
            for k, v in zc.stats(f)[1].items():
                hand[k] = hand.get(k, 0) + v
    assert hand["lit_rle"] and hand["OF_repeat"] and hand["seq_long"] and hand["seq_2byte"] and hand["skippable"]


@needs_libzstd
def test_committed_streams_equal_libzstd():
    for z in zc.libzstd_builds():
        for e in MANIFEST["streams"]:
            s = zc.load_stream(e)
            assert zc.decode(s, e["length"])[1] == z.decompress(s, e["length"]), (z.version, e["name"])


@needs_libzstd
@pytest.mark.parametrize("level", [-5, 1, 3, 9, 19, 22])
def test_fresh_compression_equals_libzstd(inputs, level):
    """Levels 19 and 22 take the inputs up to 64 KB, the label signal and the long period-7 run (libzstd needs seconds for the rest)."""
    for z in zc.libzstd_builds():
        for name, data in inputs.items():
            if level >= 19 and len(data) > (64 << 10) and name not in ("labels", "period7_210000"):
                continue
            s = z.compress(data, level)
            ref = z.decompress(s, len(data))
            assert ref == data
            n, out = zc.decode(s, len(data))
            assert n == len(data) and out == ref, (z.version, name, level)


@needs_libzstd
def test_streaming_frames_equal_libzstd(inputs):
    for z in zc.libzstd_builds():
        for name in ("labels", "image64", "rows_flipped", "period7_210000", "zeros"):
            for level, chunk in ((1, 50000), (9, 7000)):
                s = z.compress_stream(inputs[name], level, chunk)
                st = zc.stats(s)[1]
                if len(inputs[name]) > chunk:                      # (one call that also ends the frame tells libzstd the size: a one-shot frame)
                    assert st["window_desc"] >= 1 and st["single_segment"] == 0
                assert zc.decode(s, len(inputs[name]))[1] == inputs[name] == z.decompress(s, len(inputs[name])), (z.version, name, level)
        s = z.compress_advanced(inputs["image"], 3, checksum=True)
        assert zc.stats(s)[1]["checksum"] == 1 and zc.decode(s, len(inputs["image"]))[1] == inputs["image"]


def test_hand_built_frames():
    """Every header form, reserved bits, dictionary id, skippable and concatenated frames, the modes libzstd did not emit."""
    builds = zc.libzstd_builds()
    for name, (f, exp, _) in zc.hand_frames().items():
        n, out = zc.decode(f, 200000)
        if exp is None:
            assert n == _lib.ERR_INVALID, name
        else:
            assert n == len(exp) and out == exp, name
            for z in builds:                                       # the frames are no private dialect: libzstd reads the same bytes
                assert z.decompress(f, 200000) == exp, (name, z.version)


def test_committed_hand_frames_are_the_hand_built_ones():
    """The sanitizer program and the GPU tests read the hand-built frames from tests/golden/zstd; they are what hand_frames() builds."""
    built, committed = zc.hand_frames(), zc.committed_hand_frames()
    assert set(built) == set(committed)
    for name, (f, exp, host_only) in built.items():
        assert committed[name][0] == f, name
    for e in MANIFEST["hand"]:
        exp = built[e["name"]][1]
        assert e["length"] == (-1 if exp is None else len(exp)) and e["sha256"] == ("" if exp is None else zc.sha(exp)), e["name"]


def test_flip_generator_is_the_sanitizer_programs():
    """zstd_cases.flip_bits restates the sequence of csrc/checks/zstd_check.cpp (a 64-bit LCG seeded by the stream's size): the first values
    for two sizes, worked out by hand from the recurrence in Python's integers."""
    for n in (84, 15663):
        seed, want = (0x9E3779B97F4A7C15 ^ n) % 2 ** 64, []
        for _ in range(3):
            seed = (seed * 6364136223846793005 + 1442695040888963407) % 2 ** 64
            want.append((seed >> 24) % (8 * n))
        assert zc.flip_bits(n, 3) == want and all(0 <= b < 8 * n for b in zc.flip_bits(n, 4000))
    src = open(os.path.join(zc.ROOT, "treedetection_amd", "csrc", "checks", "zstd_check.cpp")).read()
    assert "0x9E3779B97F4A7C15ull ^ (uint64_t)n" in src and "6364136223846793005ull + 1442695040888963407ull" in src and "(seed >> 24) % (n * 8)" in src


def test_checksum_good_and_bad():
    e = STREAMS["image64_checksum"]
    s = zc.load_stream(e)
    assert zc.stats(s)[1]["checksum"] == 1
    assert zc.decode(s, e["length"])[0] == e["length"]
    bad = bytearray(s)
    bad[-1] ^= 0x10                                                # the stored checksum
    assert zc.decode(bytes(bad), e["length"])[0] == _lib.ERR_INVALID
    assert "checksum" in _lib.load().td_last_error().decode()
    assert zc.decode(s[:-1], e["length"])[0] == _lib.ERR_INVALID     # the stream ends inside the checksum
    # a hand-built frame whose checksum was computed by the committed stream's writer: raw block, XXH64 of b"" is 0xEF46DB3751D8E999
    empty = zc.frame(zc.block(0, b""), single=True, fcs=0, fcs_bytes=1, checksum=0x51D8E999)
    assert zc.decode(empty, 10)[0] == 0
    assert zc.decode(zc.frame(zc.block(0, b""), single=True, fcs=0, fcs_bytes=1, checksum=0x51D8E998), 10)[0] == _lib.ERR_INVALID


def test_capacity_rule():
    for name in ("image64_l9", "zeros_l9", "noise_l9", "period7_210000", "labels_stream"):
        e = STREAMS[name]
        s = zc.load_stream(e)
        assert zc.decode(s, e["length"] - 1)[0] == _lib.ERR_CAPACITY, name
        assert zc.decode(s, e["length"] // 3)[0] == _lib.ERR_CAPACITY, name
        assert zc.decode(s, 0)[0] == _lib.ERR_CAPACITY, name
        assert zc.decode(s, e["length"] + 77)[0] == e["length"], name
    two = zc.hand_frames()["two_frames"]
    assert zc.decode(two[0], len(two[1]) - 1)[0] == _lib.ERR_CAPACITY    # the second frame is the one that does not fit
    assert zc.decode(b"", 10)[0] == 0


@pytest.mark.skipif(len(zc.libzstd_builds()) < 2, reason="needs two libzstd builds: the decoder is held to the library where its builds agree")
def test_damaged_streams_against_two_builds(capsys):
    """Prefixes and seeded bit flips have no single right answer (the builds disagree on 7 % of them), so: where both builds accept a
    mutation with the same bytes, ours returns those bytes or refuses; where both refuse, an acceptance by ours is only counted. Both
    counts are printed (DESIGN.md §7 records them)."""
    a, b = zc.libzstd_builds()[:2]
    both_ok = ours_refused = both_refuse = ours_accepts = split = 0
    for name in ("image64_l9", "labels_l19_new", "rows_flipped_l9", "image16_diff_l9", "labels_stream", "image64_diff_l1_old"):
        e = STREAMS[name]
        s = zc.load_stream(e)
        for m in zc.mutations(s, seed=e["length"], prefixes=60, flips=500):
            ra, rb = a.decompress(m, e["length"]), b.decompress(m, e["length"])
            n, out = zc.decode(m, e["length"])
            assert n >= 0 or n in (_lib.ERR_INVALID, _lib.ERR_CAPACITY)
            if ra is not None and ra == rb:
                both_ok += 1
                if n < 0:
                    ours_refused += 1
                else:
                    assert out == ra, (name, len(m))
            elif ra is None and rb is None:
                both_refuse += 1
                ours_accepts += n >= 0
            else:
                split += 1
    with capsys.disabled():
        print(f"\nzstd mutations: both builds accept {both_ok} (ours refuses {ours_refused}), both refuse {both_refuse} "
              f"(ours accepts {ours_accepts}), builds disagree {split}")
    assert both_ok > 500 and both_refuse > 500


# ---- GeoTIFFs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_pillow_fallback(monkeypatch):
    def refuse(self):
        raise AssertionError("a ZSTD raster went to _pil_fallback")
    monkeypatch.setattr(GeoTiff, "_pil_fallback", refuse)


def test_committed_files(no_pillow_fallback):
    for e in MANIFEST["files"]:
        with GeoTiff(os.path.join(zc.GOLDEN, e["file"])) as g:
            assert g.compression == 50000
            px = np.ascontiguousarray(g.read().transpose(1, 2, 0))
            assert list(px.shape) == e["shape"] and str(px.dtype) == e["dtype"] and zc.sha(px.tobytes()) == e["pixel_sha256"], e["name"]
            win = g._window_hwc(37, 61, 90, 100)
            assert np.array_equal(win, px[37:127, 61:161]), e["name"]


def test_pillow_written_file_equals_pillows_decode(no_pillow_fallback):
    from PIL import Image
    path = os.path.join(zc.GOLDEN, "rgb_pillow.tif")
    with GeoTiff(path) as g:
        ours = g.read().transpose(1, 2, 0)
        n, st = zc.stats(bytes(g._mm[g._offs[0]:g._offs[0] + g._counts[0]]))
    assert st["window_desc"] >= 1                                  # libtiff writes through the streaming API
    assert np.array_equal(ours, np.asarray(Image.open(path)))


def _raster(dtype, bands, rows=150, cols=200):
    img = zc.smooth_image(seed=33, side=256, bands=bands, noise=1.0)[:rows, :cols].transpose(2, 0, 1).astype(np.int64)
    if dtype == np.uint16:
        return (img * 211 + 500).astype(np.uint16)
    if dtype == np.float32:
        return (img * 0.37 - 11.5).astype(np.float32)
    return img.astype(np.uint8)


@needs_libzstd
@pytest.mark.parametrize("dtype,bands,opts", [
    (np.uint8, 3, dict(tile=(64, 64), predictor=2)), (np.uint8, 4, dict(rows_per_strip=7)), (np.uint8, 4, dict(tile=(32, 48), predictor=1, planar=True)),
    (np.uint8, 1, dict(rows_per_strip=150, predictor=2)), (np.uint16, 3, dict(tile=(64, 64), predictor=2)), (np.uint16, 2, dict(rows_per_strip=11, planar=True, predictor=2)),
    (np.float32, 1, dict(tile=(64, 64), predictor=3)), (np.float32, 1, dict(rows_per_strip=16, predictor=2)), (np.float32, 2, dict(tile=(16, 32), predictor=1)),
])
def test_written_rasters_equal_the_uncompressed_file(tmp_path, no_pillow_fallback, dtype, bands, opts):
    arr = _raster(dtype, bands)
    pz, pu = str(tmp_path / "z.tif"), str(tmp_path / "u.tif")
    write_geotiff(pz, arr, TRANSFORM, compression="zstd", zstd_level=9, **opts)
    write_geotiff(pu, arr, TRANSFORM)
    with GeoTiff(pz) as z, GeoTiff(pu) as u:
        assert z.compression == 50000 and u.compression == 1
        assert np.array_equal(z.read(), u.read()) and np.array_equal(z.read(), arr)
        for r0, c0, h, w in ((0, 0, 150, 200), (63, 63, 3, 3), (10, 100, 140, 100), (149, 0, 1, 200)):
            assert np.array_equal(z._window_hwc(r0, c0, h, w), u._window_hwc(r0, c0, h, w))
        assert z.device_decodable(float_samples=True) == (not opts.get("planar"))
        assert z.device_decodable() == (not opts.get("planar") and dtype != np.float32)


@needs_libzstd
def test_writer_levels(tmp_path, no_pillow_fallback):
    arr = _raster(np.uint16, 1)
    for level in (1, 19):
        p = str(tmp_path / f"l{level}.tif")
        write_geotiff(p, arr, TRANSFORM, compression="zstd", zstd_level=level, rows_per_strip=50)
        with GeoTiff(p) as g:
            assert np.array_equal(g.read(), arr)


@needs_libzstd
def test_damaged_blocks_raise(tmp_path, no_pillow_fallback):
    arr = _raster(np.uint8, 3)
    p = str(tmp_path / "z.tif")
    write_geotiff(p, arr, TRANSFORM, compression="zstd", tile=(64, 64))
    with GeoTiff(p) as g:
        g._setup_blocks()
        g._counts[4] -= 1                                          # a block truncated by one byte
        with pytest.raises(ValueError, match=r"block \(0,1,0\)"):
            g._window_hwc(64, 0, 64, 64)
        assert g._window_hwc(0, 0, 64, 64).shape == (64, 64, 3)      # the other blocks still read
    # a frame that regenerates more than the block's bytes: refused (libtiff would stop reading at the block's size)
    data = bytearray(open(p, "rb").read())
    with GeoTiff(p) as g:
        g._setup_blocks()
        off, cnt = g._offs[0], g._counts[0]
    big = gt._libzstd_compressor()(bytes(64 * 64 * 3 + 1), 3)
    assert len(big) <= cnt
    data[off:off + len(big)] = big
    p2 = str(tmp_path / "big.tif")
    open(p2, "wb").write(bytes(data))
    with GeoTiff(p2) as g:
        g._setup_blocks()
        g._counts[0] = len(big)
        with pytest.raises(ValueError, match="capacity"):
            g._window_hwc(0, 0, 64, 64)


def test_writer_without_libzstd_raises(tmp_path, monkeypatch):
    import ctypes.util
    import glob
    monkeypatch.setattr(gt, "_zstd_compress", None)
    monkeypatch.setattr(ctypes.util, "find_library", lambda name: None)
    monkeypatch.setattr(glob, "glob", lambda pattern: [])
    with pytest.raises(ValueError, match="libzstd was not found"):
        write_geotiff(str(tmp_path / "z.tif"), _raster(np.uint8, 1), TRANSFORM, compression="zstd")
