"""conv_split_pack generalised to a 3x3 bank (td_conv_split_pack, taps = 9): piece p of weight (n, tap, c) lies where the split
tail's fragment read expects it (bottleneck.hip, the split form of phase 1). No GPU.

What the kernel reads: the wave that owns channel chunk cc walks k-chunks cc * 9 + tap, tap = 0 .. 8; for column tile t, slice s and
piece p it loads 1 KB at ((t * 18 + cc * 9 + tap) * 6 + 3 s + p) * 1024, 16 B per lane; lane l = (r = l & 31, h = l >> 5) multiplies
its eight bf16 (e = 0 .. 7) with the activations of channels 32 cc + 16 s + 8 (e >> 2) + 4 h + (e & 3) of that tap (the two 16-B
pieces 4 s + h and 4 s + 2 + h of the row's 128-B k-chunk) into output channel 32 t + r.

Two banks. (1) Distinct values that bf16 holds exactly — every normal bf16 bit pattern once, so piece 0 IS the weight (it names
its (n, tap, c)) and pieces 1 and 2 are zero. (2) The distinct integers 1 .. 36 864 (below 2^24: the three pieces hold them exactly):
each piece equals the round-to-nearest-even bf16 of what the earlier pieces left, and the three sum to the weight. The 1x1 form
(taps = 1) keeps its layout, columns past cout zero."""
import ctypes as C

import numpy as np

from treedetection_amd import _lib

N, TAPS, CIN = 64, 9, 64


def _pack(w, cout, cin, taps):
    lib = _lib.load()
    w = np.ascontiguousarray(w, dtype=np.float32)
    need = lib.td_conv_split_pack(w.ctypes.data_as(C.c_void_p), cout, cin, taps, None, 0)
    assert need == -(-cout // 32) * taps * (cin // 32) * 6144, need
    out = np.zeros(need // 2, dtype=np.uint16)
    assert lib.td_conv_split_pack(w.ctypes.data_as(C.c_void_p), cout, cin, taps, out.ctypes.data_as(C.c_void_p), need) == need
    return out.reshape(-(-cout // 32), taps * (cin // 32), 2, 3, 64, 8)      # [tile][k-chunk][slice][piece][lane][8]


def _bf16_rne(v):
    """float32 array -> (bf16 bits as uint16, the bf16 value as float32), round to nearest even."""
    u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    bits = u.astype(np.uint16)
    return bits, (bits.astype(np.uint32) << 16).view(np.float32)


def _expected_index(taps, cin):
    """[tile][k-chunk][slice][lane][e] -> (n, tap, channel) as the fragment read pairs them."""
    nch = taps * (cin // 32)
    t, c, s, l, e = np.meshgrid(np.arange(2), np.arange(nch), np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    n = 32 * t + (l & 31)
    cc, tap = c // taps, c % taps
    ch = 32 * cc + 16 * s + 8 * (e >> 2) + 4 * (l >> 5) + (e & 3)
    return n, tap, ch


def test_bf16_exact_bank_names_every_weight_in_piece_0():
    pats = np.arange(0x0080, 0x7F80, dtype=np.uint32)                      # every positive normal bf16
    pats = np.concatenate([pats, pats | 0x8000])[:N * TAPS * CIN]
    assert len(np.unique(pats)) == N * TAPS * CIN
    w = (pats << 16).view(np.float32).reshape(N, TAPS, CIN)
    bank = _pack(w, N, CIN, TAPS)
    n, tap, ch = _expected_index(TAPS, CIN)
    want = (w[n, tap, ch].view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(bank[:, :, :, 0], want)
    assert not bank[:, :, :, 1:].any()


def test_integer_bank_is_split_into_three_exact_pieces():
    w = np.arange(1, N * TAPS * CIN + 1, dtype=np.float32).reshape(N, TAPS, CIN)
    bank = _pack(w, N, CIN, TAPS)
    n, tap, ch = _expected_index(TAPS, CIN)
    left = w[n, tap, ch]
    total = np.zeros_like(left, dtype=np.float64)
    for p in range(3):
        bits, val = _bf16_rne(left)
        assert np.array_equal(bank[:, :, :, p], bits), p
        total += val
        left = left - val                                                  # exact
    assert np.array_equal(total, w[n, tap, ch].astype(np.float64)) and not left.any()


def test_the_1x1_form_keeps_its_layout():
    cout, cin = 40, 64
    w = np.arange(1, cout * cin + 1, dtype=np.float32).reshape(cout, 1, cin)
    bank = _pack(w, cout, cin, 1)
    n, tap, ch = _expected_index(1, cin)
    live = n < cout
    bits, _ = _bf16_rne(np.where(live, w[np.minimum(n, cout - 1), tap, ch], 0).astype(np.float32))
    assert np.array_equal(bank[:, :, :, 0], bits)
    assert not bank.transpose(0, 1, 2, 4, 5, 3)[~live].any()              # columns 40 .. 63: all three pieces zero
