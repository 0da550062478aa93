"""Launch shapes shared by the split-bf16 contraction tests (tests/test_conv_split_ref.py on the CPU, tests/test_conv_split_gpu.py
on the GPU) and the CPU emulation of conv_split_kernel's arithmetic (plain module).

The kernel (treedetection_amd/csrc/conv_split.hip) writes each fp32 operand as p0 + p1 + p2, three bf16 pieces, each the
round-to-nearest-even bf16 of what the earlier pieces left over, and accumulates six of the nine piece products per K = 16 slice
in the fp32 MFMA accumulator, small terms first: p0q2, p2q0, p1q1, p0q1, p1q0, p0q0."""
import torch

from tests import conv_ref as cr

SPLIT_IDS = (34, 35, 36)            # 128x256, 128x128, 64x256 (common.h TD_CONV_TILES)
NS = 3                              # LDS stages of conv_split_kernel's k loop = k-chunks per turn of its unrolled loop

# (layer, batch): the four short-K shapes — a ragged M with a partial 32-column tile (494 rows, 48 channels), M below one block
# with a shortcut and ReLU (15 rows), stride 2 (338 rows) and the nearest-2x shortcut (288 rows); k-chunks of 32: 2, 1, 4 = NS + 1, 8
SHORT_K = [
    (cr.Conv("s64x48", 64, 48, 1, 1, 0, 13, 19), 2),
    (cr.Conv("s32x96.res", 32, 96, 1, 1, 0, 5, 1, res=1), 3),
    (cr.Conv("s128x64.s2", 128, 64, 1, 2, 0, 26, 26), 2),
    (cr.Conv("s256x64.up2", 256, 64, 1, 1, 0, 12, 12, res=2), 2),
]

PRODUCTS = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]        # (activation piece, filter piece), in the kernel's order
DEFECTS = {
    "p2q0_dropped": [p for p in PRODUCTS if p != (2, 0)],
    "p1q1_dropped": [p for p in PRODUCTS if p != (1, 1)],
    "two_pieces_only": [p for p in PRODUCTS if 2 not in p],
}


def pieces(t: torch.Tensor, n: int = 3):
    """fp32 tensor → n bf16 pieces (as fp32 values), each the round-to-nearest-even bf16 of the remainder (exact in fp32)."""
    out, r = [], t.float()
    for _ in range(n):
        p = r.to(torch.bfloat16).float()
        out.append(p)
        r = r - p
    return out


def emulate(L: cr.Conv, inp: dict, products=PRODUCTS) -> cr.Guarded:
    """conv_split_kernel on the CPU: per K = 16 slice one fp32 accumulator update per piece product (the 16 bf16 x bf16 products
    of an MFMA are exact, their sum is taken in float64 and rounded into the fp32 accumulator), slices ascending, then the fp32
    epilogue — scale, bias, shortcut, ReLU, one IEEE operation each."""
    assert L.k == 1 and L.pad == 0 and not inp["fp16"]
    M = inp["B"] * L.Ho * L.Wo
    P = cr._patches(L, inp["x"].t, torch.arange(M))
    Wm = inp["w"].reshape(L.Cout, -1)
    pa, qb = pieces(P), pieces(Wm)
    pa64, qb64 = [p.double() for p in pa], [q.double() for q in qb]
    acc = torch.zeros(M, L.Cout, dtype=torch.float32)
    for c in range(0, L.K, 16):
        for ia, ib in products:
            acc = (acc.double() + pa64[ia][:, c:c + 16] @ qb64[ib][:, c:c + 16].T).float()
    y = acc
    if inp["scale"] is not None:
        y = y * inp["scale"].float()
    if inp["bias"] is not None:
        y = y + inp["bias"].float()
    if inp["res"] is not None:
        y = y + cr._residual_rows(L, inp["res"].t, torch.arange(M)).float()
    if L.relu:
        y = y.clamp_min(0)
    out = cr.new_output(L, inp)
    out.t.copy_(y.reshape(out.t.shape))
    return out
