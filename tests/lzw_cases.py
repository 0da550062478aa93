"""Crafted TIFF LZW code streams for the two decoders (td_tiff_lzw_decode in tiffcodec.cpp, tiff_lzw_blocks_kernel in tiffdecode.hip):
a code packer, a plain oracle, a small encoder with the policies the project's writer lacks, and the named case families. Importing
it needs neither a GPU nor the library (only host_decode at the end loads it). tests/test_lzw_cases.py holds the host decoder to the oracle and locks what the families cover;
tests/test_lzw_cases_gpu.py sends the same streams to the kernel."""
import numpy as np

CLEAR, EOI, FIRST, MAXC = 256, 257, 258, 4096
# what the kernel is built around (tests/test_lzw_cases.py ties these to the text of tiffdecode.hip)
CHUNK = 64                       # codes cut out of the stream per step
RINGS = (4096, 16384)            # bytes of recent output in LDS: small / large
REL_MAX = 65535 - 4096           # the last epoch-relative position at which the uint16 table still takes an entry
OK, CORRUPT, TOO_LONG = 0, 1, 2  # the kernel's status values; the host returns a count / TD_ERR_INVALID / TD_ERR_CAPACITY
SIZE_GROUPS = (4 << 10, 256 << 10, 8 << 20)


def pack(codes, pad_bytes: int = 0) -> bytes:
    """Codes → bytes, MSB first, at the width the DECODER expects for each: nine bits after a ClearCode (and at the start), one more when
    its next free code reaches 511 / 1023 / 2047, twelve from then on (a full table included); the first code after a ClearCode adds no
    entry. The last byte is zero-padded; ``pad_bytes`` whole zero bytes follow."""
    out, acc, have = bytearray(), 0, 0
    nbits, nxt, fresh = 9, FIRST, True
    for c in codes:
        assert 0 <= c < (1 << nbits), (c, nbits)
        acc = (acc << nbits) | c
        have += nbits
        while have >= 8:
            out.append((acc >> (have - 8)) & 255)
            have -= 8
        acc &= (1 << have) - 1
        if c == CLEAR:
            nbits, nxt, fresh = 9, FIRST, True
        elif c == EOI:
            pass
        elif fresh:
            fresh = False
        elif nxt < MAXC:
            nxt += 1
            if nxt > (1 << nbits) - 2 and nbits < 12:
                nbits += 1
    if have:
        out.append((acc << (8 - have)) & 255)
    return bytes(out) + bytes(pad_bytes)


class Decoder:
    """TIFF 6.0 §13 with the host decoder's rules, one code at a time: the table is a dict code → bytes; no output window, no prefix
    chains. Alongside it counts what the stream contains (``stats``); the positions kept per entry serve those counts only."""

    def __init__(self):
        self.out = bytearray()
        self.table, self.start = {}, {}
        self.next, self.nbits, self.old, self.old_pos, self.idx, self.epoch = FIRST, 9, None, 0, 0, 0
        self.first = True
        self.stats = {"clears": 0, "kwkwk": 0, "full_reads": 0, "max_len": 0, "max_epoch": 0, "eoi": False, "leading_clear": False,
                      "max_dist": 0, "max_add_at": -1, "length": 0, "far": {r: 0 for r in RINGS}, "lens": set(),
                      "at": {k: set() for k in ("clear", "eoi", "end", "corrupt", "kwkwk")}, "refs": {}}

    def length(self, code: int) -> int:
        return 1 if code < 256 else len(self.table[code])

    def feed(self, code: int):
        """→ None (go on), OK (EOI) or CORRUPT."""
        st = self.stats
        first, self.first = self.first, False
        if code == EOI:
            st["eoi"] = True
            st["at"]["eoi"].add(self.idx)
            return OK
        if code == CLEAR:
            st["clears"] += 1
            st["leading_clear"] |= first
            st["at"]["clear"].add(self.idx)
            self.table, self.start = {}, {}
            self.next, self.nbits, self.old, self.idx = FIRST, 9, None, 0
            return None
        op = len(self.out)
        if self.old is None:                                       # the first code after a clear (or of the stream): a literal
            if code > 255:
                st["at"]["corrupt"].add(self.idx)
                return CORRUPT
            self.epoch, self.old, self.old_pos, self.idx = op, bytes([code]), op, 1
            self.out.append(code)
            st["lens"].add(1)
            st["max_len"] = max(st["max_len"], 1)
            st["max_epoch"] = max(st["max_epoch"], 1)
            return None
        if code < 256:
            s = bytes([code])
        elif code in self.table:
            s = self.table[code]
            dist = op - self.start[code]
        elif code == self.next and self.next < MAXC:               # KwKwK: the entry this very code defines
            s = self.old + self.old[:1]
            dist = op - self.old_pos
            st["kwkwk"] += 1
            st["at"]["kwkwk"].add(self.idx)
        else:
            st["at"]["corrupt"].add(self.idx)
            return CORRUPT
        if self.next == MAXC:
            st["full_reads"] += 1
        if code > 255:
            st["max_dist"] = max(st["max_dist"], dist)
            d = self.idx + 257 - code                              # the entry was defined d codes ago (0: by this one)
            if d <= 70:
                st["refs"].setdefault(d, set()).add(self.idx)
            for r in RINGS:                                        # the code-by-code loop's rule for leaving the ring (tiffdecode.hip)
                st["far"][r] += len(s) > 64 or dist + 64 > r
        if self.next < MAXC:
            st["max_add_at"] = max(st["max_add_at"], op - self.epoch)
            self.table[self.next] = self.old + s[:1]
            self.start[self.next] = self.old_pos
            self.next += 1
            if self.next > (1 << self.nbits) - 2 and self.nbits < 12:
                self.nbits += 1
        self.out += s
        self.old, self.old_pos = s, op
        self.idx += 1
        st["lens"].add(len(s))
        st["max_len"] = max(st["max_len"], len(s))
        st["max_epoch"] = max(st["max_epoch"], len(self.out) - self.epoch)
        return None


def oracle(stream: bytes, cap: int):
    """→ (status, bytes, stats). Input that ends without EOI is accepted; more than ``cap`` bytes is TOO_LONG with the ``cap`` bytes that
    fit (stats["length"] is the whole length); a corrupt code wins over both."""
    d = Decoder()
    padded = stream + b"\0\0\0"
    pos, total, status = 0, len(stream) * 8, OK
    while True:
        nb = d.nbits
        if pos + nb > total:
            d.stats["at"]["end"].add(d.idx)
            break
        three = int.from_bytes(padded[pos >> 3:(pos >> 3) + 3], "big")
        code = (three >> (24 - (pos & 7) - nb)) & ((1 << nb) - 1)
        pos += nb
        r = d.feed(code)
        if r is not None:
            status = r
            break
    d.stats["length"] = len(d.out)
    if status == CORRUPT:
        return CORRUPT, b"", d.stats
    if len(d.out) > cap:
        return TOO_LONG, bytes(d.out[:cap]), d.stats
    return OK, bytes(d.out), d.stats


def encode_codes(data: bytes, clear_at=None, leading_clear: bool = True, eoi: bool = True):
    """An LZW encoder with other policies than the writer's: a ClearCode after every ``clear_at`` codes, or never (``None``: once the table
    is full the stream goes on at twelve bits with the entries it has — the deferred clear of TIFF 6.0), no leading ClearCode, no EOI."""
    codes = [CLEAR] if leading_clear else []
    table, nxt, since = {}, FIRST, 0
    if data:
        cur = data[0]
        for c in data[1:]:
            hit = table.get((cur, c))
            if hit is not None:
                cur = hit
                continue
            codes.append(cur)
            since += 1
            if nxt < MAXC:
                table[(cur, c)] = nxt
                nxt += 1
            if clear_at is not None and since >= clear_at:
                codes.append(CLEAR)
                table, nxt, since = {}, FIRST, 0
            cur = c
        codes.append(cur)
    if eoi:
        codes.append(EOI)
    return codes


def encode(data: bytes, clear_at=None, leading_clear: bool = True, eoi: bool = True) -> bytes:
    return pack(encode_codes(data, clear_at, leading_clear, eoi))


class Build:
    """A code list under construction, with a Decoder beside it that tells the generators where the stream stands."""

    def __init__(self, *codes):
        self.codes, self.d = [], Decoder()
        self.put(*codes)

    def put(self, *codes):
        for c in codes:
            self.codes.append(c)
            assert self.d.feed(c) is None, c
        return self

    def literals(self, rng, n: int):
        return self.put(*(int(v) for v in rng.integers(0, 256, n)))

    def mixed(self, rng, n: int, max_len: int = 2):
        """n codes: literals and, about one in three, an entry of at most ``max_len`` bytes — string starts are no longer code indices."""
        for _ in range(n):
            short = [c for c in range(max(FIRST, self.d.next - 40), self.d.next) if len(self.d.table[c]) <= max_len]
            if self.d.old is not None and short and rng.random() < 0.35:
                self.put(short[int(rng.integers(0, len(short)))])
            else:
                self.put(int(rng.integers(0, 256)))
        return self

    def climb(self, length: int):
        """KwKwK codes until the last string is ``length`` bytes long (after one literal: 2, 3, 4, ...)."""
        while len(self.d.old) < length:
            self.put(self.d.next)
        return self

    @property
    def op(self) -> int:
        return len(self.d.out)

    def stream(self, *tail, pad_bytes: int = 0) -> bytes:
        """The stream with ``tail`` behind it — codes the Decoder here need not accept."""
        return pack(self.codes + list(tail), pad_bytes)

    def copy(self):
        b = Build()
        b.put(*self.codes)
        return b


EVENTS = ("clear", "eoi", "end", "beyond", "max", "kwkwk", "prev", "prev2")


def event_streams(b: Build, name: str, out: dict) -> None:
    """The events of the sweeps behind the codes of ``b``: ClearCode + two literals + EOI; EOI; the end of the input; the code one beyond the
    table; the largest code of the current width (4095 at twelve bits — at nine bits 4095 has no encoding; beyond the table except where
    the table is full); KwKwK; the entry the previous code defined; the one before it. The last three go on with a literal and EOI."""
    nxt, nbits = b.d.next, b.d.nbits
    out[f"{name}/clear"] = b.stream(CLEAR, 7, 9, EOI)
    out[f"{name}/eoi"] = b.stream(EOI)
    out[f"{name}/end"] = b.stream()
    if nxt + 1 < (1 << nbits):
        out[f"{name}/beyond"] = b.stream(nxt + 1)
    out[f"{name}/max"] = b.stream((1 << nbits) - 1, 5, EOI)
    if nxt < MAXC:
        out[f"{name}/kwkwk"] = b.stream(nxt, 200, EOI)
    if nxt - 1 >= FIRST:
        out[f"{name}/prev"] = b.stream(nxt - 1, 201, EOI)
    if nxt - 2 >= FIRST:
        out[f"{name}/prev2"] = b.stream(nxt - 2, 202, EOI)


def trivial() -> dict:
    out = {"empty": b"", "eoi_only": pack([EOI]), "clear_eoi": pack([CLEAR, EOI]), "clear_clear_eoi": pack([CLEAR, CLEAR, EOI]),
           "clear_nonliteral_258": pack([CLEAR, 258]), "clear_nonliteral_300": pack([CLEAR, 300, 65, EOI]),
           "clear_lit_clear_nonliteral": pack([CLEAR, 65, CLEAR, 258, EOI]),
           "no_leading_clear": pack([65, 66, 67, 258, 260, EOI]), "no_leading_clear_kwkwk": pack([97, 258, 259, EOI]),
           "one_literal": pack([CLEAR, 65, EOI]), "a_258": pack([CLEAR, 97, 258, EOI]), "a_258_no_eoi": pack([CLEAR, 97, 258])}
    for n in range(1, 9):                                          # n nine-bit codes leave (-9 n) mod 8 pad bits: 7, 6, ..., 0
        codes = [CLEAR] + [64 + k for k in range(n - 1)]
        out[f"no_eoi_pad_bits_{(-9 * n) % 8}"] = pack(codes)
    for extra in (1, 4):                                           # whole zero bytes: nine zero bits are the literal 0
        out[f"no_eoi_pad_bytes_{extra}"] = pack([CLEAR, 65, 66, 258], pad_bytes=extra)
        out[f"eoi_pad_bytes_{extra}"] = pack([CLEAR, 65, 66, 258, EOI], pad_bytes=extra)
    return out


def event_sweeps() -> dict:
    """k = 1 .. 130 codes after a ClearCode, then each event: every stop and every in-chunk reference at every lane of a 64-code chunk,
    twice over. 'lit': literals (a string starts at its code's index); 'mix': short strings among them (it does not)."""
    out = {}
    rng = np.random.default_rng(2024)
    for k in range(1, 131):
        event_streams(Build(CLEAR).literals(rng, k), f"lit{k}", out)
        event_streams(Build(CLEAR).mixed(rng, k), f"mix{k}", out)
    return out


def in_chunk_distance() -> dict:
    """A code that names the entry defined d codes earlier, d = 1 .. 70 — inside the same chunk up to 63, whatever the chunk's start."""
    out = {}
    rng = np.random.default_rng(77)
    for d in range(1, 71):
        for k in (d + 1, 100):
            if k > d:
                b = Build(CLEAR).mixed(rng, k)
                out[f"d{d}_k{k}"] = b.stream(257 + k - d, 33, 257 + k - d, EOI)
    return out


WIDTH_EDGES = (253, 254, 255, 765, 766, 767, 1789, 1790, 1791)
FULL = MAXC - FIRST + 1                                            # 3 839 codes after a ClearCode fill the table (the first adds no entry)


def width_edges() -> dict:
    out = {}
    rng = np.random.default_rng(5)
    for k in WIDTH_EDGES:
        event_streams(Build(CLEAR).literals(rng, k), f"lit{k}", out)
        event_streams(Build(CLEAR).mixed(rng, k), f"mix{k}", out)
    # around the full table: libtiff's encoder clears after 3 837 codes (the decoder's next free code is 4094)
    for n in (FULL - 2, FULL - 1, FULL, FULL + 1):
        b = Build(CLEAR).literals(rng, n)
        out[f"lits{n}_clear"] = b.stream(CLEAR, 1, 2, 258, EOI)
        out[f"lits{n}_eoi"] = b.stream(EOI)
        out[f"lits{n}_end"] = b.stream()
    b = Build(CLEAR).literals(rng, FULL)
    assert b.d.next == MAXC
    more = [int(v) for v in rng.integers(0, MAXC - 2, 300)]
    more = [c + 2 if c >= CLEAR else c for c in more]              # any literal or entry, never ClearCode / EOI
    more[17] = more[250] = MAXC - 1
    out["full_then_300"] = b.copy().put(*more).stream(EOI)
    out["full_then_300_clear"] = b.copy().put(*more).stream(CLEAR, 3, 4, 258, EOI)
    out["full_then_4096"] = b.stream(5, 6, MAXC - 1, 7)            # (twelve bits cannot say 4096: the largest code is a valid one here)
    return out


KWKWK_LENGTHS = (63, 64, 65, 128, 129, 2048, 2049, 3838, 3839)


def kwkwk_runs() -> dict:
    """a 258 259 ...: every code names the entry it defines; the last string is n bytes long (3 839: code 4095, the longest there is)."""
    out = {}
    for n in KWKWK_LENGTHS:
        b = Build(CLEAR, 97).climb(n)
        out[f"run{n}"] = b.stream(EOI)
        if n <= 129:
            out[f"run{n}_then_first"] = b.stream(258, 98, b.d.next - 1, EOI)
    return out


def _ring_prefix():
    """ClearCode, 'a' 'b' (entry 258 = "ab" begins at the epoch's first byte), then a climb to a 60-byte string: the filler."""
    b = Build(CLEAR, 97, 98, 99).climb(60)
    return b, b.d.next - 1


def _fill_to(b: Build, filler: int, target: int):
    """Strings of 60 bytes, then literals, until the output stands at ``target``: no string over 64 bytes on the way."""
    while target - b.op >= 60:
        b.put(filler)
    while b.op < target:
        b.put(100 + (b.op % 50))
    return b


def ring_distances() -> dict:
    """A code that names entry 258 when the output stands D bytes behind the entry's start, D = RING - 130 .. RING + 2: around the
    code-by-code rule (D + 64 <= RING) and, in the middle of 64 ordinary codes, around the chunk's (its END - source <= RING). No string
    of these streams is longer than 64 bytes, so only the distance sends a copy through memory. Then one run of 64 strings whose sum
    lies at RING / 2 - 1 .. RING / 2 + 1, after 0 .. 63 other codes."""
    out = {}
    base, filler = _ring_prefix()
    for ring in RINGS:
        for dist in range(ring - 130, ring + 3):
            b = _fill_to(base.copy(), filler, dist)
            out[f"ring{ring}_d{dist}"] = b.stream(258, 65, EOI)
            b = _fill_to(base.copy(), filler, dist - 32)
            b.put(*range(1, 33))
            assert b.op == dist
            out[f"ring{ring}_d{dist}_mid"] = b.stream(258, *range(40, 71), EOI)
        # 64 strings that sum to RING / 2 + delta: entries of the climb (entry 257 + m is m + 1 bytes long)
        per = ring // 2 // 64
        clim = Build(CLEAR, 97).climb(per + 8)
        for delta in (-1, 0, 1):
            for lead in range(0, 64, 9):
                b = clim.copy().put(*([98] * lead))
                lens = [per] * 63 + [per + delta]
                out[f"ring{ring}_half{delta:+d}_lead{lead}"] = b.stream(*(257 + n - 1 for n in lens), 99, EOI)
    return out


def _edge_epoch(lits: int) -> Build:
    """349 KwKwK codes after 'a' give 61 425 bytes; ``lits`` literals behind them arrive at 61 425, 61 426, ..."""
    b = Build(CLEAR, 97).climb(350)
    assert b.op == 61425
    return b.put(*([98] * lits))


def sixteen_bit_edge() -> dict:
    out = {}
    out["add_at_61439"] = _edge_epoch(15).stream(EOI)              # the last table-adding code arrives at REL_MAX: narrow table
    out["add_at_61440"] = _edge_epoch(16).stream(EOI)              # one byte more: wide pass
    out["add_at_61440_goes_on"] = _edge_epoch(16).stream(258, 259, 98, EOI)
    out["clear_at_61439"] = _edge_epoch(14).stream(CLEAR, 1, 2, 258, EOI)
    out["clear_at_61440"] = _edge_epoch(15).stream(CLEAR, 1, 2, 258, EOI)
    out["eoi_at_61440"] = _edge_epoch(15).stream(EOI)
    out["string_across_61439"] = _edge_epoch(10).stream(300, EOI)   # begins below REL_MAX, ends beyond it; nothing follows
    out["string_across_61439_then_add"] = _edge_epoch(10).stream(300, 98, EOI)
    for name, n in (("past_65536", 365), ("past_131072", 515)):    # flat climbs that then name their earliest entries
        b = Build(CLEAR, 97).climb(n)
        out[name] = b.stream(258, 259, 98, 258, b.d.next - 1, EOI)
    return out


def real_inputs() -> dict:
    rng = np.random.default_rng(11)
    t = np.arange(40000)
    smooth = (128 + 60 * np.sin(t / 47.0) + 30 * np.sin(t / 5.3) + rng.integers(-1, 2, t.size)).astype(np.uint8)
    return {"smooth": smooth.tobytes(), "noise4": rng.integers(0, 4, 30000, dtype=np.uint8).tobytes(),
            "period251": np.resize(rng.integers(0, 256, 251, dtype=np.uint8), 20000).tobytes()}


REAL_POLICIES = {"clear300": {"clear_at": 300}, "clear511": {"clear_at": 511}, "clear1023": {"clear_at": 1023}, "clear3000": {"clear_at": 3000},
                 "never": {"clear_at": None}, "never_no_eoi": {"clear_at": None, "eoi": False},
                 "clear511_no_leading": {"clear_at": 511, "leading_clear": False},
                 "never_bare": {"clear_at": None, "leading_clear": False, "eoi": False}}


def real_data() -> dict:
    """name → (stream, the bytes it was made from)."""
    return {f"{name}_{pol}": (encode(data, **kw), data) for name, data in real_inputs().items() for pol, kw in REAL_POLICIES.items()}


FAMILIES = {"trivial": trivial, "event_sweeps": event_sweeps, "in_chunk_distance": in_chunk_distance, "width_edges": width_edges,
            "kwkwk_runs": kwkwk_runs, "ring_distances": ring_distances, "sixteen_bit_edge": sixteen_bit_edge,
            "real_data": lambda: {k: v[0] for k, v in real_data().items()}}
_cache = {}


def family(name: str) -> dict:
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def all_cases() -> dict:
    """"family/name" → stream, every family."""
    return {f"{fam}/{name}": s for fam in FAMILIES for name, s in family(fam).items()}


def judged(name: str, stream: bytes, cap: int):
    """oracle(), kept per (case, capacity): the CPU and the GPU tests of one process judge a stream once."""
    key = ("judged", name, cap)
    if key not in _cache:
        _cache[key] = oracle(stream, cap)
    return _cache[key]


def size_groups() -> list:
    """The cases by decoded size (<= 4 KB, <= 256 KB, <= 8 MB) → [(capacity, {name: stream})]: one launch per group keeps blocks x
    capacity small. The capacity is the group's longest output and 64 bytes, so that every case of the group fits."""
    groups = [{} for _ in SIZE_GROUPS]
    for name, s in all_cases().items():
        n = judged(name, s, SIZE_GROUPS[-1])[2]["length"]
        groups[next(i for i, lim in enumerate(SIZE_GROUPS) if n <= lim)][name] = s
    return [(max(judged(n, s, SIZE_GROUPS[-1])[2]["length"] for n, s in g.items()) + 64, g) for g in groups]


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
MUTATION_CAP = 3000                                               # below the length of four of the six sources


def mutation_sources() -> dict:
    """Six streams under 20 KB: three encodings of real data, a KwKwK run, short strings, a copy from the far end of the small ring."""
    inp = real_inputs()
    rng = np.random.default_rng(9)
    return {"smooth_clear300": encode(inp["smooth"][:6000], clear_at=300), "noise4_never": encode(inp["noise4"][:9000]),
            "period251_bare": encode(inp["period251"][:2500], clear_at=1023, leading_clear=False, eoi=False),
            "run129": family("kwkwk_runs")["run129_then_first"], "mixed900": Build(CLEAR).mixed(rng, 900, max_len=6).stream(EOI),
            "ring4096": family("ring_distances")["ring4096_d4040_mid"]}


def mutations(stream: bytes, seed: int, step: int = 97, flips: int = 40) -> list:
    """Every ``step``-th prefix and ``flips`` seeded single-bit flips."""
    rng = np.random.default_rng(seed)
    out = [stream[:cut] for cut in range(0, len(stream), step)]
    for pos in (int(v) for v in rng.integers(0, len(stream) * 8, flips)):
        b = bytearray(stream)
        b[pos >> 3] ^= 0x80 >> (pos & 7)
        out.append(bytes(b))
    return out


def mutation_cases() -> dict:
    if "mutations" not in _cache:
        out = {}
        for k, (name, s) in enumerate(mutation_sources().items()):
            assert len(s) < 20000, name
            for j, m in enumerate(mutations(s, 100 + k)):
                out[f"mutations/{name}/{j}"] = m
        _cache["mutations"] = out
    return _cache["mutations"]


def host_decode(stream: bytes, cap: int):
    """td_tiff_lzw_decode → (status, count, its output buffer [cap + 16]: 0xA5 where it wrote nothing)."""
    from treedetection_amd import _lib
    src = np.frombuffer(stream, dtype=np.uint8).copy() if stream else np.zeros(1, np.uint8)
    dst = np.full(cap + 16, 0xA5, dtype=np.uint8)
    n = int(_lib.load().td_tiff_lzw_decode(src.ctypes.data, len(stream), dst.ctypes.data, cap))
    return {_lib.ERR_INVALID: CORRUPT, _lib.ERR_CAPACITY: TOO_LONG}.get(n, OK), n, dst


def host_agrees(name: str, stream: bytes, cap: int):
    """The host decoder against the oracle: status, count, bytes; under TOO_LONG the part that fits; nothing behind the capacity."""
    status, data, stats = judged(name, stream, cap)
    hs, n, dst = host_decode(stream, cap)
    assert hs == status, (name, cap, hs, n, status)
    assert (dst[cap:] == 0xA5).all(), name
    if status == OK:
        assert n == len(data) and dst[:n].tobytes() == data and (dst[n:] == 0xA5).all(), (name, cap, n, len(data))
    elif status == TOO_LONG:
        assert dst[:cap].tobytes() == data, (name, cap)
    return status, data, stats
