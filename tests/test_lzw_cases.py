"""The host LZW decoder (td_tiff_lzw_decode, tiffcodec.cpp) held to the oracle of tests/lzw_cases.py on every crafted stream and
mutation, and the locks that keep those streams what tests/test_lzw_cases_gpu.py takes them for: what each family reaches, the
kernel constants they are built around, and libtiff reading the valid ones the same way."""
import io
import os
import struct

import numpy as np
import pytest

import lzw_cases as lc
from treedetection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats_of(fam: str) -> dict:
    return {name: lc.judged(f"{fam}/{name}", s, lc.SIZE_GROUPS[-1]) for name, s in lc.family(fam).items()}


def test_packer_and_encoder_reproduce_the_writers_streams():
    """pack() and encode() against the project's writer: td_tiff_lzw_encode clears when its own next free code reaches 4095, that is
    after 3 837 codes — the same policy here must give the same bytes."""
    lib = _lib.load()
    for name, data in lc.real_inputs().items():
        src = np.frombuffer(data, dtype=np.uint8)
        dst = np.empty(len(data) * 2 + 64, dtype=np.uint8)
        n = lib.td_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, dst.size)
        assert dst[:n].tobytes() == lc.encode(data, clear_at=lc.FULL - 2), name
    assert lc.pack([lc.CLEAR, 7, 7, 258, lc.EOI]) == bytes([0x80, 0x01, 0xC0, 0xF0, 0x28, 0x08])   # 9-bit codes 256 7 7 258 257, MSB first, by hand
    assert lc.pack([lc.CLEAR], pad_bytes=2) == b"\x80\x00\x00\x00"


def test_real_data_under_other_policies_decodes_to_its_input():
    for name, (s, data) in lc.real_data().items():
        status, out, stats = lc.judged(f"real_data/{name}", s, lc.SIZE_GROUPS[-1])
        assert status == lc.OK and out == data, name
        assert stats["eoi"] == ("no_eoi" not in name and "bare" not in name), name
        assert stats["leading_clear"] == ("no_leading" not in name and "bare" not in name), name
        if "never" in name and not name.startswith("period251"):
            assert stats["clears"] <= 1 and stats["full_reads"] > 1000, name
        if name.endswith("clear300"):
            assert stats["clears"] > 20, name


def test_host_decoder_equals_the_oracle_on_every_case():
    seen = {lc.OK: 0, lc.CORRUPT: 0, lc.TOO_LONG: 0}
    for cap, cases in lc.size_groups():
        for k, (name, s) in enumerate(cases.items()):
            status, data, stats = lc.host_agrees(name, s, cap)
            seen[status] += 1
            if status == lc.OK and len(data) > 1 and (k % 23 == 0 or len(data) > lc.SIZE_GROUPS[1]):
                for small in (len(data) - 1, len(data) // 3, 1, 0):
                    assert lc.host_agrees(name, s, small)[0] == lc.TOO_LONG, (name, small)
    assert seen[lc.OK] > 2000 and seen[lc.CORRUPT] > 500 and seen[lc.TOO_LONG] == 0, seen


def test_host_decoder_equals_the_oracle_on_the_mutations():
    """Every 97th prefix and 40 single-bit flips of six streams, at a capacity below four of them. A condition on the inputs, met by the
    oracle alone: each of the three outcomes occurs at least ten times."""
    seen = {lc.OK: 0, lc.CORRUPT: 0, lc.TOO_LONG: 0}
    for name, s in lc.mutation_cases().items():
        seen[lc.judged(name, s, lc.MUTATION_CAP)[0]] += 1
    assert min(seen.values()) >= 10, seen
    assert sum(len(lc.oracle(s, 1 << 20)[1]) > lc.MUTATION_CAP for s in lc.mutation_sources().values()) == 4
    for name, s in lc.mutation_cases().items():
        lc.host_agrees(name, s, lc.MUTATION_CAP)


def test_families_reach_what_they_claim():
    """A later edit to the generators cannot thin the coverage: the oracle's counts show what each family is there for."""
    # trivial
    t = stats_of("trivial")
    assert t["empty"][0] == lc.OK and t["empty"][2]["length"] == 0 and t["clear_clear_eoi"][2]["clears"] == 2
    assert t["clear_nonliteral_258"][0] == t["clear_nonliteral_300"][0] == t["clear_lit_clear_nonliteral"][0] == lc.CORRUPT
    assert not t["no_leading_clear"][2]["leading_clear"] and t["no_leading_clear"][1] == b"ABCABCA"
    assert t["a_258"][1] == b"aaa" and t["a_258"][2]["at"]["kwkwk"] == {1}                    # KwKwK as the second code: lane 0 of the first chunk
    assert t["no_leading_clear_kwkwk"][1] == b"aaaaaa"
    assert sorted(n for n in t if n.startswith("no_eoi_pad_bits_")) == [f"no_eoi_pad_bits_{k}" for k in range(8)]
    assert all(not t[f"no_eoi_pad_bits_{k}"][2]["eoi"] and t[f"no_eoi_pad_bits_{k}"][0] == lc.OK for k in range(8))
    assert t["no_eoi_pad_bytes_4"][1] == b"ABAB\0\0\0\0" and t["eoi_pad_bytes_4"][1] == b"ABAB"
    # event sweeps: every stop and every near reference at every code index 1 .. 130 — every lane, whatever the chunk's start
    for kind in ("lit", "mix"):
        at = {k: set() for k in ("clear", "eoi", "end", "corrupt", "kwkwk", 1, 2)}
        for name, (status, data, st) in stats_of("event_sweeps").items():
            if name.startswith(kind):
                for k in ("clear", "eoi", "end", "corrupt", "kwkwk"):
                    at[k] |= st["at"][k]
                for d in (1, 2):
                    at[d] |= st["refs"].get(d, set())
                ev = name.split("/")[1]
                assert status == (lc.CORRUPT if ev in ("beyond", "max") else lc.OK), name
        want = set(range(1, 131))
        assert at["clear"] >= want and at["eoi"] >= want and at["end"] >= want and at["corrupt"] >= want and at["kwkwk"] >= want, kind
        assert at[1] >= want - {1} and at[2] >= want - {1, 2}, kind
    mixed = [st for name, (_, _, st) in stats_of("event_sweeps").items() if name.startswith("mix")]
    assert sum(st["max_len"] > 1 for st in mixed) > 900           # (string starts differ from code indices)
    # in-chunk distance: d = 1 .. 70, each at two code indices
    refs = {}
    for status, data, st in stats_of("in_chunk_distance").values():
        assert status == lc.OK
        for d, idx in st["refs"].items():
            refs.setdefault(d, set()).update(idx)
    assert all({d + 1, 100} <= refs[d] for d in range(1, 71)), refs
    # width edges: events exactly on, before and behind the three changes of width; the full table with and without a ClearCode
    w = stats_of("width_edges")
    for ev in lc.EVENTS:
        idx = set()
        for name, (status, data, st) in w.items():
            if name.endswith("/" + ev):
                idx |= {int(name.split("/")[0][3:])}
                key = {"beyond": "corrupt", "max": "corrupt", "prev": None, "prev2": None}.get(ev, ev)
                if key:
                    assert int(name.split("/")[0][3:]) in st["at"][key], name
        assert idx == set(lc.WIDTH_EDGES), (ev, idx)
    assert lc.FULL == 3839 and w[f"lits{lc.FULL - 1}_eoi"][2]["full_reads"] == 0 and w[f"lits{lc.FULL}_eoi"][2]["full_reads"] == 0
    assert w[f"lits{lc.FULL + 1}_eoi"][2]["full_reads"] == 1 and w[f"lits{lc.FULL + 1}_clear"][0] == lc.OK
    assert w[f"lits{lc.FULL - 2}_clear"][2]["at"]["clear"] == {0, lc.FULL - 2}                 # where libtiff's encoder puts it
    assert w["full_then_300"][0] == lc.OK and w["full_then_300"][2]["full_reads"] == 300 and w["full_then_300"][2]["clears"] == 1
    assert w["full_then_300_clear"][2]["clears"] == 2 and w["full_then_4096"][2]["full_reads"] == 4
    # KwKwK runs: string lengths on both sides of 64 and of 2 048, and the longest string there is
    kw = stats_of("kwkwk_runs")
    assert [kw[f"run{n}"][2]["max_len"] for n in lc.KWKWK_LENGTHS] == list(lc.KWKWK_LENGTHS) == [63, 64, 65, 128, 129, 2048, 2049, 3838, 3839]
    assert all(kw[f"run{n}"][2]["kwkwk"] == n - 1 and kw[f"run{n}"][1] == b"a" * (n * (n + 1) // 2) for n in lc.KWKWK_LENGTHS)
    assert kw["run3839"][2]["max_add_at"] < 2 ** 31 and kw["run3839"][2]["full_reads"] == 0
    # ring distances: sources at every distance RING - 130 .. RING + 2, no string over 64 bytes; 64 strings around RING / 2
    r = stats_of("ring_distances")
    for ring in lc.RINGS:
        for mid in ("", "_mid"):
            got = {}
            for name, (status, data, st) in r.items():
                if name.startswith(f"ring{ring}_d") and name.endswith("_mid") == bool(mid):
                    assert status == lc.OK and st["max_len"] <= 64 and st["max_dist"] == int(name.split("_")[1][1:]), name
                    got[st["max_dist"]] = st["far"][ring]
            assert sorted(got) == list(range(ring - 130, ring + 3)), (ring, mid)
            assert all((got[d] > 0) == (d + 64 > ring) for d in got), (ring, mid)              # on both sides of the code-by-code rule
        half = {name: v for name, v in r.items() if name.startswith(f"ring{ring}_half")}
        assert len(half) == 24
        for name, (status, data, st) in half.items():
            lead, delta = int(name.split("lead")[1]), int(name.split("half")[1].split("_")[0])
            assert status == lc.OK and data[-1 - (ring // 2 + delta):-1] == b"a" * (ring // 2 + delta) and data[-1:] == b"c", name
            assert {ring // 2 // 64, ring // 2 // 64 + delta} <= st["lens"], name
    # the sixteen-bit edge
    e = stats_of("sixteen_bit_edge")
    assert lc.REL_MAX == 61439
    assert e["add_at_61439"][2]["max_add_at"] == 61439 and e["add_at_61440"][2]["max_add_at"] == 61440 and e["add_at_61440_goes_on"][2]["max_add_at"] > 61440
    assert e["clear_at_61439"][2]["max_add_at"] == 61438 and e["clear_at_61439"][2]["max_epoch"] == 61439
    assert e["clear_at_61440"][2]["max_add_at"] == 61439 and e["clear_at_61440"][2]["max_epoch"] == 61440 and e["eoi_at_61440"][2]["max_epoch"] == 61440
    assert e["string_across_61439"][2]["max_add_at"] == 61435 and e["string_across_61439"][2]["max_epoch"] > 61440
    assert e["string_across_61439_then_add"][2]["max_add_at"] > 61440
    assert 65536 < e["past_65536"][2]["max_epoch"] < 131072 < e["past_131072"][2]["max_epoch"]
    assert e["past_131072"][2]["max_dist"] > 131072 and all(v[0] == lc.OK for v in e.values())
    wide = {name for name, v in e.items() if v[2]["max_add_at"] > lc.REL_MAX}
    assert wide == {"add_at_61440", "add_at_61440_goes_on", "string_across_61439_then_add", "past_65536", "past_131072"}
    # the size groups: the 8-MB group is a handful of blocks
    groups = lc.size_groups()
    assert [cap <= lim + 64 for (cap, _), lim in zip(groups, lc.SIZE_GROUPS)] == [True] * 3 and 1 <= len(groups[2][1]) <= 6
    assert sum(len(g) for _, g in groups) == len(lc.all_cases()) > 3000


def test_case_constants_are_the_kernels():
    """64 codes per chunk, rings of 4 096 and 16 384 bytes, REL_MAX, and the two rules the oracle's counts restate (when the code-by-code
    loop leaves the ring; when a block goes to the wide pass): the text of tiffdecode.hip that defines them."""
    src = open(os.path.join(ROOT, "treedetection_amd", "csrc", "tiffdecode.hip")).read()
    assert lc.CHUNK == 64 and "uint32_t n = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;" in src and "const uint32_t idx = c0 + lane;" in src
    assert lc.RINGS == (4096, 16384) and "TD_LZW(4096, true, 12)" in src and "TD_LZW(4096, false, 12)" in src
    assert "TD_LZW(16384, true, 6)" in src and "TD_LZW(16384, false, 6)" in src and "tiff_lzw_blocks_kernel<uint32_t, true, 16384, true, 4>" in src
    assert lc.REL_MAX == 65535 - 4096 and "REL_MAX = sizeof(TableT) == 2 ? 65535u - 4096u : 0xffffffffu;" in src
    assert "if (op - epoch > REL_MAX) {" in src
    assert "s_len <= 64 && (code < 256 || op - s_start + 64 <= (uint32_t)LZW_RING)" in src
    assert "incl > (uint32_t)LZW_RING / 2u" in src and "op_end - src <= (uint32_t)LZW_RING" in src
    assert 'getenv("TD_DECODE_RING")' in src and 'getenv("TD_LZW_ONE_BY_ONE")' in src


def one_strip_tiff(stream: bytes, n: int) -> bytes:
    """A minimal little-endian TIFF: one row of n 8-bit grey pixels in one LZW strip."""
    tags = [(256, 4, n), (257, 4, 1), (258, 3, 8), (259, 3, 5), (262, 3, 1), (273, 4, 8 + 2 + 9 * 12 + 4), (277, 3, 1), (278, 4, 1), (279, 4, len(stream))]
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, typ, 1, v) for t, typ, v in tags) + struct.pack("<I", 0)
    return struct.pack("<2sHI", b"II", 42, 8) + ifd + stream


def test_libtiff_reads_the_valid_canonical_streams_alike():
    """The crafted streams are no private dialect: each valid one with a leading ClearCode and EOI, as the only strip of a grey TIFF,
    decodes under libtiff (through Pillow) to the oracle's bytes. One limit is libtiff's own: its decoder goes on adding entries behind
    code 4095 into 1 024 spare slots, and refuses the stream ("Using code not yet in table") when they are used up — a deferred clear of
    more than about a thousand codes. Those streams (two encodings of real data that never clear) are left out of THIS check only;
    the 300 codes behind a full table, code 4095 among them, are in it."""
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    done = 0
    for cap, cases in lc.size_groups():
        for name, s in cases.items():
            status, data, st = lc.judged(name, s, cap)
            if status != lc.OK or not (st["leading_clear"] and st["eoi"]) or not data or st["full_reads"] >= 1000:
                continue
            with Image.open(io.BytesIO(one_strip_tiff(s, len(data)))) as im:
                assert im.tobytes() == data, name
            done += 1
    assert done > 1500
    refused = [n for n, s in lc.all_cases().items() if lc.judged(n, s, lc.SIZE_GROUPS[-1])[2]["full_reads"] >= 1000]
    assert all(n.startswith("real_data/") and "_never" in n for n in refused) and len(refused) <= 6, refused
    assert lc.judged("width_edges/full_then_300", lc.family("width_edges")["full_then_300"], lc.SIZE_GROUPS[-1])[2]["full_reads"] == 300
