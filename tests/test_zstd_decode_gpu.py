"""Zstandard blocks decoded on the GPU (zstddecode.hip: zstd_core.h on a 64-lane wave per block) against the same core on a host thread
(td_tiff_zstd_decode) and the hashes of the committed streams. Nothing here needs libzstd: the streams, the hand-built frames and
the five GeoTIFFs are in tests/golden/zstd and tests/zstd_cases.py."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import zstd_cases as zc
from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu
MANIFEST = zc.manifest()
CANARY = 0xA5


def host(stream: bytes, cap: int):
    """td_tiff_zstd_decode → (status or count, its whole output buffer [cap])."""
    lib = _lib.load()
    src = np.frombuffer(stream, dtype=np.uint8).copy() if stream else np.zeros(1, np.uint8)
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    return int(lib.td_tiff_zstd_decode(src.ctypes.data, len(stream), dst.ctypes.data, cap)), dst


def launch(streams, cap, scratch_bytes=None, stream=None):
    """All streams as the blocks of ONE launch → (status, decoded, rows [n + 1, cap]: a canary row behind the last block)."""
    lib = _lib.load()
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s
    blob += b"\0" * 16
    n = len(streams)
    comp = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_n = torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")
    out = torch.full((n + 1, cap), CANARY, dtype=torch.uint8, device="cuda")
    dec = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    need = int(lib.td_tiff_zstd_scratch_bytes(n))
    assert need > 0
    scratch = torch.empty((scratch_bytes or need,), dtype=torch.uint8, device="cuda")
    _lib.check(lib.td_tiff_zstd_decode_dev(comp.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), n, out.data_ptr(), cap, dec.data_ptr(), status.data_ptr(),
                                           scratch.data_ptr(), scratch.numel(), _lib.stream_ptr()), "td_tiff_zstd_decode_dev")
    torch.cuda.synchronize()
    return status.cpu().numpy(), dec.cpu().numpy(), out.cpu().numpy()


def header_declines(s: bytes) -> bool:
    """True where the device declines a block at its first frame's header (status 4) whatever follows: a skippable frame in front, or a
    well-formed frame header (reserved bit clear, dictionary id zero, all its bytes there) with the content-checksum flag — a bit flip
    can set that flag; the host wrapper then reads on and decides (a stream without the four checksum bytes is corrupt to it)."""
    if len(s) >= 4 and (int.from_bytes(s[:4], "little") & 0xFFFFFFF0) == 0x184D2A50:
        return True
    if len(s) < 6 or s[:4] != zc.MAGIC or s[4] & 0x08 or not s[4] & 0x04:
        return False
    single, did = s[4] >> 5 & 1, (0, 1, 2, 4)[s[4] & 3]
    fcs = (single, 2, 4, 8)[s[4] >> 6]
    at = 5 + (0 if single else 1)
    return len(s) >= at + did + fcs and not any(s[at:at + did]) and not (not single and s[5] >> 3 > 31)


def compare(names, streams, cap, declined=()):
    """Device against host, case by case: 0 ↔ the same bytes; 1 ↔ TD_ERR_INVALID; 2 ↔ TD_ERR_CAPACITY and the part that fits is the
    host's; 4 only where the host wrapper's extras are in play (``declined``)."""
    refs = [host(s, cap) for s in streams]                         # the host function first: nothing reaches the kernel that it has not returned from
    st, dec, rows = launch(streams, cap)
    assert (rows[len(streams)] == CANARY).all(), "the row behind the last block was written"
    counts = {0: 0, 1: 0, 2: 0, 4: 0}
    for i, (name, s) in enumerate(zip(names, streams)):
        n, ref = refs[i]
        counts[int(st[i])] += 1
        if name in declined or header_declines(s):
            assert st[i] == 4, (name, st[i])
        elif n >= 0 and len(s) > 0:
            assert st[i] == 0 and dec[i] == n and np.array_equal(rows[i, :n], ref[:n]), (name, st[i], dec[i], n)
            assert (rows[i, n:] == CANARY).all(), name
        elif n == _lib.ERR_CAPACITY:
            assert st[i] == 2 and dec[i] > cap and np.array_equal(rows[i], ref[:cap]), (name, st[i], dec[i])
        else:
            assert st[i] == 1, (name, st[i], n)
    return counts


def test_committed_streams_and_hand_built_frames_in_one_launch():
    names, streams, declined = [], [], set()
    for e in MANIFEST["streams"]:
        names.append(e["name"])
        streams.append(zc.load_stream(e))
        if e["api"] == "checksum":
            declined.add(e["name"])
    for name, (f, exp, host_only) in zc.committed_hand_frames().items():       # (the bytes the sanitizer program runs over)
        names.append(name)
        streams.append(f)
        if host_only:
            declined.add(name)
    cap = max(e["length"] for e in MANIFEST["streams"])
    assert cap == 300000                                           # ZSTD_CHECK_HAND_CAP of csrc/checks/zstd_check.cpp: the hand-built frames ran with it
    counts = compare(names, streams, cap, declined)
    st, dec, rows = launch(streams, cap)
    for i, e in enumerate(MANIFEST["streams"]):                     # the manifest's hashes, straight from the device's bytes
        if e["name"] not in declined:
            assert st[i] == 0 and dec[i] == e["length"] and zc.sha(rows[i, :e["length"]].tobytes()) == e["sha256"], (e["name"], st[i], dec[i])
    assert counts[4] == len(declined) and counts[1] >= 8 and counts[0] >= 45


def test_prefixes_and_bit_flips_equal_the_host_case_by_case():
    """≈ 300 prefixes and single-bit flips of six committed streams in one launch, every one of them a case the sanitizer program
    (make zstd-check) has run on the host: it runs every prefix, its first 40 flips per stream are zstd_cases.flip_bits' (one
    generator), and it runs these streams with this capacity (ZSTD_CHECK_SMALL_CAP) too. The capacity is below four of the streams'
    lengths: those that still decode end with status 2."""
    names, streams = [], []
    for name in ("image64_l9", "labels_l19_new", "rows_flipped_l9", "image16_diff_l9", "labels_stream", "period65_700"):
        e = next(x for x in MANIFEST["streams"] if x["name"] == name)
        s = zc.load_stream(e)
        assert len(s) <= 20000                                     # (the program runs the small capacity for streams up to that size)
        for k, m in enumerate([s] + zc.mutations(s, seed=7 + e["length"], prefixes=9, flips=40)):
            names.append(f"{name}#{k}")
            streams.append(m)
    assert 280 <= len(streams) <= 320
    counts = compare(names, streams, 20000)
    assert counts[0] >= 20 and counts[1] >= 50 and counts[2] >= 3 and counts[4] == sum(header_declines(s) for s in streams) <= 3, counts


def test_more_blocks_than_decoder_waves_go_by_ticket():
    """3 000 small blocks: more than the chip holds decoder waves. Again with the scratch of ONE workgroup, so that eight waves take them all."""
    lib = _lib.load()
    small = [e for e in MANIFEST["streams"] if e["length"] <= 1024]
    assert len(small) >= 10
    names = [small[i % len(small)]["name"] + f"#{i}" for i in range(3000)]
    streams = [zc.load_stream(small[i % len(small)]) for i in range(3000)]
    one_group = int(lib.td_tiff_zstd_scratch_bytes(1))
    for scratch in (None, one_group):
        st, dec, rows = launch(streams, 1024, scratch_bytes=scratch)
        assert (st == 0).all() and (rows[3000] == CANARY).all()
        for i in range(3000):
            e = small[i % len(small)]
            assert dec[i] == e["length"], names[i]
        for j, e in enumerate(small):                               # every copy of a stream gives the manifest's bytes
            got = rows[j:3000:len(small), :e["length"]]
            assert zc.sha(got[0].tobytes()) == e["sha256"] and (got == got[0]).all(), e["name"]


def test_decode_to_device_equals_the_host_reader_also_on_the_low_priority_stream():
    low = _lib.low_priority_stream(0)
    a = torch.randn((4096, 4096), device="cuda")
    pinned = [None]
    for e in MANIFEST["files"]:
        path = os.path.join(zc.GOLDEN, e["file"])
        with GeoTiff(path) as g:
            ref = np.ascontiguousarray(g.read().transpose(1, 2, 0))
        assert zc.sha(ref.tobytes()) == e["pixel_sha256"]
        for stream in (None, low):
            busy = torch.tanh(a * 1.0001) + a                       # other work on the current stream while the decode runs
            with GeoTiff(path) as g:
                assert g.device_decodable(float_samples=True)
                image, check = g.decode_to_device("cuda:0", stream, pinned)
                busy = torch.tanh(busy) * a
                got = check().cpu()
            got = got.view(torch.int16).numpy().view(np.uint16) if got.dtype == torch.uint16 else got.numpy()
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (e["name"], stream is low)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(busy).any())


def _predict(tmp_path, tag, tif, device_decode, sd):
    import treedetection_amd as TD
    from treedetection_amd.preprocessing import tile_single_file
    d = tmp_path / tag
    tile_single_file(tif, str(d / "tiles"), buffer=2, tile_width=15, tile_height=15)
    name = os.path.splitext(os.path.basename(tif))[0]
    cfg = TD.setup_model_cfg(update_model="x", device="0")
    with TD.Predictor(cfg, device_type="0", max_batch_size=3, output_dir=str(d / "out"), state_dict=sd, device_decode=device_decode) as pred:
        pred(tif, str(d / "tiles" / f"{name}.json"))
        images = pred.decode_stats["images"]
    out = d / "out" / name
    files = sorted(os.listdir(out)) if out.exists() else []
    return images, {f: open(out / f, "rb").read() for f in files}


def test_prediction_files_are_identical_with_the_device_decoder_on_or_off(tmp_path):
    """A ZSTD raster (four bands, strips) through the Predictor: windows cut in HBM (device_decode true) against the block-wise host
    reader (false) — byte-identical Prediction files. "auto" sends ZSTD rasters to the device as it does LZW and DEFLATE ones."""
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    tif = str(tmp_path / "9.tif")
    shutil.copy(os.path.join(zc.GOLDEN, "rgbi_strips7.tif"), tif)
    on_images, on = _predict(tmp_path, "on", tif, True, sd)
    off_images, off = _predict(tmp_path, "off", tif, False, sd)
    auto_images, auto = _predict(tmp_path, "auto", tif, "auto", sd)
    assert on_images == 1 and off_images == 0 and auto_images == 1
    assert len(on) >= 4 and on == off == auto


def test_a_damaged_block_is_reported_by_number_and_the_predictor_falls_back(tmp_path, capsys):
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    good = os.path.join(zc.GOLDEN, "rgbi_strips7.tif")
    with GeoTiff(good) as g:
        g._setup_blocks()
        off = g._offs[5]
    raw = bytearray(open(good, "rb").read())
    raw[off + 1: off + 4] = b"\xff\xff\xff"                         # block 5 no longer begins with a frame
    bad = str(tmp_path / "bad.tif")
    open(bad, "wb").write(bytes(raw))
    with GeoTiff(bad) as g:
        image, check = g.decode_to_device("cuda:0")
        with pytest.raises(ValueError, match="block 5"):
            check()
    images, files = _predict(tmp_path, "bad", bad, True, sd)
    assert images == 0 and "using the host reader" in capsys.readouterr().out
    good_images, good_files = _predict(tmp_path, "good", good, True, sd)
    assert good_images == 1 and 0 < len(files) < len(good_files)     # the host reader rejects the same block: the tiles that need it are dropped
