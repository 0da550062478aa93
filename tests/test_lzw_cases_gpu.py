"""The GPU LZW decoder (tiff_lzw_blocks_kernel, tiffdecode.hip) held to the oracle of tests/lzw_cases.py on crafted code streams: all four
instantiations of the first pass (ring of 16 KB / 4 KB x 64 codes per step / code by code) and the wide-table pass behind them. Every
stream has gone through the oracle and the host decoder (tests/test_lzw_cases.py) before it reaches the kernel; the high half of
``decoded`` (strings copied through memory) and the wide-pass list show that the streams reach the paths they were built for."""
import struct

import numpy as np
import pytest
import torch

import lzw_cases as lc
from treedetection_amd import _lib
from treedetection_amd.geotiff import GeoTiff, write_geotiff
from treedetection_amd.synth import make_tile

pytestmark = pytest.mark.gpu
CANARY = 0xA5
LIMIT = lc.SIZE_GROUPS[-1]


@pytest.fixture(params=[("large", None), ("large", "1"), ("small", None), ("small", "1")], ids=["ring16k-chunks", "ring16k-one_by_one", "ring4k-chunks", "ring4k-one_by_one"])
def config(request, monkeypatch):
    """→ (bytes of the ring, whether the 64-codes-per-step path runs): both are read from the environment on every call."""
    ring, one = request.param
    monkeypatch.setenv("TD_DECODE_RING", ring)
    if one is None:
        monkeypatch.delenv("TD_LZW_ONE_BY_ONE", raising=False)
    else:
        monkeypatch.setenv("TD_LZW_ONE_BY_ONE", one)
    return (lc.RINGS[1] if ring == "large" else lc.RINGS[0]), one is None


def launch(streams, cap):
    """All streams as the blocks of ONE td_tiff_lzw_decode_dev launch, their offsets cycling through the four byte alignments, 16 zero
    bytes behind the blob → (status [n], bytes produced [n], strings through memory [n], the wide-pass list as a set, rows [n + 1, cap]:
    0xA5 where nothing was written, one spare row behind the last block)."""
    lib = _lib.load()
    offs, blob = [], bytearray()
    for k, s in enumerate(streams):
        blob += b"\xff" * ((k - len(blob)) % 4)
        offs.append(len(blob))
        blob += s
    blob += b"\0" * 16
    n = len(streams)
    comp = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    assert comp.data_ptr() % 4 == 0 and [o % 4 for o in offs[:4]] == [0, 1, 2, 3][:n]
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_n = torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")
    out = torch.full((n + 1, cap), CANARY, dtype=torch.uint8, device="cuda")
    dec = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((2 * n + 1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.td_tiff_lzw_decode_dev(comp.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), n, out.data_ptr(), cap, dec.data_ptr(), status.data_ptr(),
                                          _lib.stream_ptr()), "td_tiff_lzw_decode_dev")
    torch.cuda.synchronize()
    st, dec = status.cpu().numpy(), dec.cpu().numpy()
    nwide = int(st[n])
    assert 0 <= nwide <= n
    wide = set(int(v) for v in st[n + 1:n + 1 + nwide])
    assert len(wide) == nwide and (st[n + 1 + nwide:] == -1).all()
    return st[:n], dec & 0xFFFFFFFF, dec >> 32, wide, out.cpu().numpy()


def compare(cases: dict, cap: int, ring: int, chunks: bool, keys: dict = None):
    """Device against oracle, case by case. ``keys``: case name → the name its oracle result is kept under (copies of one stream)."""
    names, streams = list(cases), list(cases.values())
    refs = [lc.host_agrees((keys or {}).get(nm, nm), s, cap) for nm, s in cases.items()]      # oracle and host first: nothing reaches the kernel that they have not judged
    st, count, slow, wide, rows = launch(streams, cap)
    assert (rows[len(streams)] == CANARY).all(), "the row behind the last block was written"
    seen = {lc.OK: 0, lc.CORRUPT: 0, lc.TOO_LONG: 0}
    for i, name in enumerate(names):
        status, data, stats = refs[i]
        seen[status] += 1
        assert st[i] == status, (name, st[i], status)
        if status == lc.OK:
            assert count[i] == len(data) and rows[i, :len(data)].tobytes() == data, (name, count[i], len(data))
            assert (rows[i, len(data):] == CANARY).all(), name
        elif status == lc.TOO_LONG:
            assert count[i] == stats["length"] > cap and rows[i].tobytes() == data, (name, count[i], stats["length"])
        # strings through memory: none where every string is short and every source near (a chunk writes at most RING / 2 bytes, so a
        # source RING / 2 back is still in the ring at the chunk's end); some where a string is over 64 bytes or a source beyond the
        # ring; code by code exactly the count of the loop's own rule. A block of the wide pass was decoded there: chunks, large ring.
        r, by_chunks = (lc.RINGS[1], True) if i in wide else (ring, chunks)
        if stats["max_len"] <= 64 and stats["max_dist"] <= r // 2:
            assert slow[i] == 0, (name, slow[i])
        if stats["max_len"] > 64 or stats["max_dist"] > r:
            assert slow[i] > 0, (name, slow[i])
        if not by_chunks:
            assert slow[i] == stats["far"][r], (name, slow[i], stats["far"][r])
    # the wide pass takes exactly the blocks in which a table-adding code arrived beyond the last position the uint16 table holds
    assert wide == {i for i in range(len(names)) if refs[i][2]["max_add_at"] > lc.REL_MAX}, [names[i] for i in wide]
    return seen, wide


@pytest.mark.parametrize("group", [0, 1, 2], ids=["to4KB", "to256KB", "to8MB"])
def test_crafted_streams_equal_the_oracle(group, config):
    ring, chunks = config
    cap, cases = lc.size_groups()[group]
    seen, wide = compare(cases, cap, ring, chunks)
    names = list(cases)
    if group == 0:
        assert seen[lc.OK] > 1800 and seen[lc.CORRUPT] > 500 and not wide
    if group == 1:
        on = {names[i] for i in wide}
        assert {"sixteen_bit_edge/add_at_61440", "sixteen_bit_edge/past_65536", "sixteen_bit_edge/past_131072"} <= on
        assert not on & {"sixteen_bit_edge/add_at_61439", "sixteen_bit_edge/clear_at_61439", "sixteen_bit_edge/clear_at_61440"}
    if group == 2:
        assert 1 <= len(cases) <= 6 and len(wide) == len(cases)      # the flat climbs: every one outgrows the narrow table
    # a few streams of the group again, in blocks that are too small for them
    ok = [nm for nm in names if lc.judged(nm, cases[nm], cap)[0] == lc.OK and lc.judged(nm, cases[nm], cap)[2]["length"] > 3]
    few = {nm: cases[nm] for nm in ok[::max(1, len(ok) // 4)][:5]}
    assert len(few) >= min(4, len(ok))
    for nm, s in few.items():
        n = lc.judged(nm, s, cap)[2]["length"]
        for small in (n - 1, n // 3):
            seen, _ = compare({nm: s}, small, ring, chunks)
            assert seen[lc.TOO_LONG] == 1
    seen, _ = compare(few, 1, ring, chunks)
    assert seen[lc.TOO_LONG] == len(few)


def test_mutations_equal_the_oracle(config):
    """Prefixes and single-bit flips of six streams in blocks of 3 000 bytes: decodes / corrupt / too long, as the oracle says."""
    ring, chunks = config
    seen, _ = compare(lc.mutation_cases(), lc.MUTATION_CAP, ring, chunks)
    assert min(seen.values()) >= 10, seen


def test_ticket_loop_on_crafted_streams(config):
    """About 3 000 blocks — more than the chip holds decoder waves, so every wave takes several from the launch's counter and reuses its
    LDS: copies of every 19th event-sweep stream, valid and corrupt ones side by side. Every copy decodes as the first."""
    ring, chunks = config
    sweeps = lc.family("event_sweeps")
    picked = list(sweeps)[::19]
    cases, keys = {}, {}
    for copy in range(27):
        for nm in picked:
            cases[f"{nm}#{copy}"] = sweeps[nm]
            keys[f"{nm}#{copy}"] = f"event_sweeps/{nm}"
    assert len(cases) > 2900
    cap = max(lc.judged(f"event_sweeps/{nm}", sweeps[nm], LIMIT)[2]["length"] for nm in picked) + 16
    seen, wide = compare(cases, cap, ring, chunks, keys)
    assert seen[lc.OK] >= 27 * 60 and seen[lc.CORRUPT] >= 27 * 15 and seen[lc.TOO_LONG] == 0 and not wide


def test_a_file_with_blocks_of_other_encoders_through_the_real_path(tmp_path, config):
    """An LZW GeoTIFF of the project's writer in which three tiles are replaced — in the file's bytes: appended, offsets and byte counts
    repointed — by encodings the writer never emits: a ClearCode every 511 codes, no ClearCode at all (deferred), no EOI."""
    rgb, _ = make_tile(21, 256)
    img = np.ascontiguousarray(rgb[:200, :250].transpose(2, 0, 1))
    path = str(tmp_path / "mixed.tif")
    write_geotiff(path, img, (0.2, 0.0, 412000.0, 0.0, -0.2, 5318100.0), 25832, compression="lzw", tile=(64, 64))
    g = GeoTiff(path)
    g._setup_blocks()
    raw = bytearray(open(path, "rb").read())
    (nent,) = struct.unpack_from("<H", raw, 8)
    where = {}
    for k in range(nent):
        tag, typ, cnt, val = struct.unpack_from("<HHII", raw, 10 + 12 * k)
        if tag in (324, 325):
            assert typ == 4 and cnt == len(g._offs) == 16
            where[tag] = val
    deferred = 0
    for blk, kw in ((3, {"clear_at": 511}), (6, {"clear_at": None}), (9, {"clear_at": lc.FULL - 2, "eoi": False})):
        status, pixels, _ = lc.oracle(bytes(raw[g._offs[blk]:g._offs[blk] + g._counts[blk]]), 64 * 64 * 3)
        assert status == lc.OK and len(pixels) == 64 * 64 * 3
        s = lc.encode(pixels, **kw)
        status, again, stats = lc.oracle(s, len(pixels))
        assert status == lc.OK and again == pixels and stats["eoi"] == kw.get("eoi", True)
        deferred += stats["full_reads"] if kw["clear_at"] is None else 0
        raw += b"\0" * (len(raw) % 2)
        struct.pack_into("<I", raw, where[324] + 4 * blk, len(raw))
        struct.pack_into("<I", raw, where[325] + 4 * blk, len(s))
        raw += s
    assert deferred > 100                                          # (the tile fills the table: the deferred clear is real)
    open(path, "wb").write(bytes(raw))
    image, check = GeoTiff(path).decode_to_device("cuda:0")
    got = check().cpu().numpy().transpose(2, 0, 1)
    assert np.array_equal(got, GeoTiff(path).read()) and np.array_equal(got, img)
