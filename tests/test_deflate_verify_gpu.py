"""The Adler-32 trailer of DEFLATE blocks decoded on the GPU (tiffdecode.hip: tiff_adler32_blocks_kernel behind
tiff_inflate_blocks_kernel): the position-parallel checksum equals zlib.adler32, td_tiff_inflate_verified_dev gives every block the
outcome zlib gives its stream, GeoTiff.decode_to_device reports a block whose bytes inflate to the right length but not to the
stream's checksum — as the host reader's zlib does — and the Predictor then serves that image through the host reader."""
import os
import zlib

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile
from treedetection_amd.weights import make_synthetic_state_dict

from deflate_cases import flipped, flips, valid_streams

pytestmark = pytest.mark.gpu
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0)


@pytest.fixture(params=["large", "small"])
def ring(request, monkeypatch):
    """Both LDS footprints of the DEFLATE decoder (32 KB / 8 KB of recent output per wave)."""
    monkeypatch.setenv("TD_DECODE_RING", request.param)
    return request.param


def _adler_dev(lib, t):
    out = torch.full((1,), -1, dtype=torch.int32, device="cuda")           # (the checksum's 32 bits)
    _lib.check(lib.td_adler32_dev(t.data_ptr(), t.numel(), out.data_ptr(), _lib.stream_ptr()), "td_adler32_dev")
    torch.cuda.synchronize()
    return int(out.cpu().numpy().view(np.uint32)[0])


def test_adler32_on_the_device_equals_zlib():
    """Lengths around the wave (64), zlib's own reduction period (5552), the modulus (65521) and the 16-byte vectors; buffers that begin
    at every offset of a 16-byte line; 64 MiB of 0xFF — the largest sums there are — and 64 MiB of noise."""
    lib = _lib.load()
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1 << 20) + 3 + 16, dtype=np.uint8)
    d_base = torch.from_numpy(base).cuda()
    for n in (0, 1, 63, 64, 65, 5552, 5553, 65520, 65521, 65522, (1 << 20) + 3):
        for start in ((0, 1, 5, 15, 16) if n < 70000 else (0, 3)):
            assert _adler_dev(lib, d_base[start:start + n]) == zlib.adler32(base[start:start + n].tobytes()), (n, start)
    ones = torch.full((64 << 20,), 0xff, dtype=torch.uint8, device="cuda")
    assert _adler_dev(lib, ones) == zlib.adler32(b"\xff" * (64 << 20))
    assert _adler_dev(lib, ones[7:(64 << 20) - 2]) == zlib.adler32(b"\xff" * ((64 << 20) - 9))
    del ones
    noise = np.random.default_rng(12).integers(0, 256, 64 << 20, dtype=np.uint8)
    assert _adler_dev(lib, torch.from_numpy(noise).cuda()) == zlib.adler32(noise.tobytes())


def _batch(streams):
    offs, blob = [], bytearray()
    for st in streams:
        blob += b"\0" * ((-len(blob)) % 3)                      # odd alignments on purpose
        offs.append(len(blob))
        blob += st
    blob += b"\0" * 16
    comp = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_n = torch.tensor([len(st) for st in streams], dtype=torch.int64, device="cuda")
    return comp, d_off, d_n


def _decode(lib, streams, cap, verified):
    comp, d_off, d_n = _batch(streams)
    nb = len(streams)
    out = torch.zeros((nb, cap), dtype=torch.uint8, device="cuda")
    dec = torch.zeros((nb,), dtype=torch.int64, device="cuda")
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    if verified:
        ends = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
        _lib.check(lib.td_tiff_inflate_verified_dev(comp.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), nb, out.data_ptr(), cap, dec.data_ptr(),
                                                    status.data_ptr(), ends.data_ptr(), _lib.stream_ptr()), "td_tiff_inflate_verified_dev")
    else:
        _lib.check(lib.td_tiff_inflate_dev(comp.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), nb, out.data_ptr(), cap, dec.data_ptr(),
                                           status.data_ptr(), _lib.stream_ptr()), "td_tiff_inflate_dev")
    torch.cuda.synchronize()
    return out, dec.cpu().numpy(), status.cpu().numpy()


def test_valid_streams_pass_the_check_with_the_plain_decoders_bytes(ring):
    lib = _lib.load()
    streams, raws = valid_streams()
    cap = max(len(r) for r in raws) + 64
    out_v, dec_v, st_v = _decode(lib, streams, cap, True)
    out_p, dec_p, st_p = _decode(lib, streams, cap, False)
    assert (st_v == 0).all() and (st_p == 0).all(), (st_v.tolist(), st_p.tolist())
    assert np.array_equal(dec_v, dec_p) and dec_v.tolist() == [len(r) for r in raws]
    assert torch.equal(out_v, out_p)
    got = out_v.cpu().numpy()
    for k, raw in enumerate(raws):
        assert got[k, :len(raw)].tobytes() == raw, k
    # a byte count that includes padding behind the trailer (the trailer is read where the last block ends, not at the end), and one
    # that ends inside the trailer (zlib: incomplete stream)
    padded = [s + b"\0\0\0" for s in streams]
    short = [s[:-1] for s in streams]
    assert (_decode(lib, padded, cap, True)[2] == 0).all()
    assert (_decode(lib, short, cap, True)[2] == 3).all()
    assert (_decode(lib, short, cap, False)[2] == 0).all()             # (the plain decoder does not look that far)


def test_every_flipped_bit_has_the_hosts_outcome_on_the_device(ring):
    """The mutated streams of tests/test_deflate_verify.py in ONE launch: per block 0 where td_tiff_inflate_verified accepts (same bytes),
    3 exactly where it says the checksum is wrong, 1 / 2 where it says corrupt / capacity. (The host function is held to zlib there.)"""
    lib = _lib.load()
    streams, raws = valid_streams()
    cap = max(len(r) for r in raws) + 64
    muts = flips(streams)
    cases = [flipped(streams[k], b) for k, b in muts]
    hbuf = np.zeros(cap + 16, dtype=np.uint8)
    host, host_bytes = [], {}
    for i, s in enumerate(cases):
        src = np.frombuffer(s, dtype=np.uint8)
        n = int(lib.td_tiff_inflate_verified(src.ctypes.data, len(s), hbuf.ctypes.data, cap))
        if n >= 0:
            host.append(0)
            host_bytes[i] = hbuf[:n].tobytes()
        elif n == _lib.ERR_CAPACITY:
            host.append(2)
        else:
            host.append(3 if b"Adler-32" in lib.td_last_error() else 1)
    host = np.array(host)
    assert (host == 3).sum() >= 32 * len(streams) and (host == 1).sum() > 100 and (host == 0).sum() >= 5
    out, dec, st = _decode(lib, cases, cap, True)
    differ = np.nonzero(st != host)[0]
    assert differ.size == 0, [(muts[i], int(st[i]), int(host[i])) for i in differ[:10]]
    for i, want in host_bytes.items():
        assert int(dec[i]) == len(want) and out[i, :len(want)].cpu().numpy().tobytes() == want, muts[i]


def _imagery(bands, h, w, seed):
    rgb, _ = make_tile(seed, max(h, w))
    return np.concatenate([rgb, rgb[..., 1:2]], axis=2)[:h, :w, :bands].transpose(2, 0, 1).copy()


def _corrupt_copy(good, bad, block, where):
    """Copy `good` with one change inside `block`'s stream: where = "trailer" flips one bit of its Adler-32, "payload" one byte of a
    stored block's bytes. → the block's stream as it now lies in the file, and the size it must decode to (asserted: zlib says
    "incorrect data check", and the decoder that stops at the last end-of-block symbol returns the block's full length)."""
    lib = _lib.load()
    g = GeoTiff(good)
    g._setup_blocks()
    off, cnt = int(g._offs[block]), int(g._counts[block])
    g.close()
    raw = bytearray(open(good, "rb").read())
    full = len(zlib.decompress(bytes(raw[off:off + cnt])))
    if where == "trailer":
        raw[off + cnt - 2] ^= 0x10
    else:
        assert (raw[off + 2] >> 1) & 3 == 0 and int.from_bytes(raw[off + 3:off + 5], "little") > 200      # a stored block comes first
        raw[off + 2 + 5 + 150] ^= 0xff
    open(bad, "wb").write(bytes(raw))
    stream = bytes(raw[off:off + cnt])
    with pytest.raises(zlib.error, match="incorrect data check"):
        zlib.decompress(stream)
    src = np.frombuffer(stream, dtype=np.uint8)
    buf = np.zeros(full + 16, dtype=np.uint8)
    assert lib.td_tiff_inflate(src.ctypes.data, len(stream), buf.ctypes.data, full) == full
    assert lib.td_tiff_inflate_verified(src.ctypes.data, len(stream), buf.ctypes.data, full) == _lib.ERR_INVALID


@pytest.mark.parametrize("where", ["trailer", "payload"])
def test_a_block_that_fails_its_checksum_is_reported_by_check(tmp_path, where):
    """(a) imagery, one bit of block 5's trailer flipped; (b) noise — zlib stores it — with one payload byte of block 6 flipped. Both
    blocks inflate to their full size: only the checksum tells. The untouched files decode as the host reader reads them."""
    if where == "trailer":
        img, block = _imagery(3, 500, 500, seed=9), 5
    else:
        img, block = np.random.default_rng(4).integers(0, 256, (3, 500, 500), dtype=np.uint8), 6
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, img, T, 25832, compression="deflate", tile=(128, 128))
    _corrupt_copy(good, bad, block, where)
    image, check = GeoTiff(bad).decode_to_device("cuda:0")
    with pytest.raises(ValueError, match=f"block {block}: Adler-32 mismatch"):
        check()
    image, check = GeoTiff(good).decode_to_device("cuda:0")
    got = check().cpu().numpy().transpose(2, 0, 1)
    assert np.array_equal(got, img) and np.array_equal(got, GeoTiff(good).read())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_untouched_predictor_2_files_still_decode_as_the_host_reader_reads_them(tmp_path, dtype, ring):
    """The checksum covers the decoder's raw output — differences under predictor 2 — for one- and two-byte samples, tiles and strips."""
    img = _imagery(4, 517, 683, seed=3).astype(dtype) * (257 if dtype == np.uint16 else 1)
    for name, kw in (("tiles", {"tile": (128, 128)}), ("strips", {"rows_per_strip": 7})):
        path = str(tmp_path / f"{name}.tif")
        write_geotiff(path, img, T, 25832, compression="deflate", predictor=2, **kw)
        image, check = GeoTiff(path).decode_to_device("cuda:0")
        got = check().cpu().numpy().transpose(2, 0, 1)
        assert got.dtype == dtype and np.array_equal(got, img) and np.array_equal(got, GeoTiff(path).read()), name


def test_the_predictor_serves_a_checksum_corrupt_image_through_the_host_reader(tmp_path, capsys):
    """Two images, one with a trailer-corrupt block, with the device decoder on and off: the good image's prediction files are
    byte-identical, and so is what becomes of the bad one — the device decoder reports the block, the host reader's zlib raises on it, the
    tiles that need it are dropped (reference prediction.py:174-176) and the others are predicted."""
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    img = _imagery(3, 500, 500, seed=9)
    good, bad = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif")
    write_geotiff(good, img, T, 25832, compression="deflate", tile=(128, 128))
    _corrupt_copy(good, bad, 5, "trailer")
    for tif in (good, bad):
        tile_single_file(tif, str(tmp_path / "tiles"), buffer=0, tile_width=25, tile_height=25)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    outs, logs = {}, {}
    for tag, dd in (("dev", "auto"), ("host", False)):
        with TD.Predictor(cfg, device_type="0", max_batch_size=4, output_dir=str(tmp_path / tag), state_dict=sd, device_decode=dd) as pred:
            for name, tif in (("good", good), ("bad", bad)):
                pred(tif, str(tmp_path / "tiles" / f"{name}.json"))
            assert pred.decode_stats["images"] == (1 if tag == "dev" else 0)
        logs[tag] = capsys.readouterr().out
        outs[tag] = {name: {f: open(tmp_path / tag / name / f, "rb").read() for f in sorted(os.listdir(tmp_path / tag / name))}
                     for name in ("good", "bad")}
    assert "Adler-32 mismatch" in logs["dev"] and "using the host reader" in logs["dev"] and "using the host reader" not in logs["host"]
    assert "incorrect data check" in logs["dev"] and "incorrect data check" in logs["host"]
    assert len(outs["dev"]["good"]) == 16 and outs["dev"]["good"] == outs["host"]["good"]
    assert 0 < len(outs["dev"]["bad"]) < 16 and outs["dev"]["bad"] == outs["host"]["bad"]
