"""The numerics of the unfolded F(4x4,3x3) form with its 36 plane contractions on split-bf16 (conv_split.hip's batched launch),
emulated in numpy / torch on the CPU: fp32 input transform B^T d B, the filter bank U = G g G^T in float64 rounded once (as
wino43_filter_transform), each plane V[p] [T x C] . U[p]^T with the kernel's three-piece / six-product arithmetic (the emulation of
tests/conv_split_cases.py), fp32 output transform A^T M A. Compared against float64 conv2d on the inputs of
test_winograd_f4x4_conv_matches_torch (mostly positive x, w / sqrt(9 C)) at C = 256, a 12 x 12 map, N = 64: within the project's
F(4x4) tolerance 5e-5 * max(1, max|ref|), printed beside the error of the same code with fp32 planes."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_split_cases import PRODUCTS, pieces

BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def plane_split(v: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """conv_split_kernel on one plane: v [T][C] . u [N][C]^T, per K = 16 slice one fp32 accumulator update per piece product"""
    pa, qb = [p.double() for p in pieces(v)], [q.double() for q in pieces(u)]
    acc = torch.zeros(v.shape[0], u.shape[0], dtype=torch.float32)
    for c in range(0, v.shape[1], 16):
        for ia, ib in PRODUCTS:
            acc = (acc.double() + pa[ia][:, c:c + 16] @ qb[ib][:, c:c + 16].T).float()
    return acc


def plane_fp32(v: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """the fp32 MFMA's chain: k ascending, two k per accumulator update (v_mfma_f32_32x32x2_f32), every product and sum rounded to fp32"""
    acc = torch.zeros(v.shape[0], u.shape[0], dtype=torch.float32)
    for c in range(0, v.shape[1], 2):
        acc = (acc + v[:, c:c + 1] * u[:, c].unsqueeze(0)) + v[:, c + 1:c + 2] * u[:, c + 1].unsqueeze(0)
    return acc


def wino43(x: np.ndarray, w: np.ndarray, plane) -> np.ndarray:
    """x [C][H][W], w [N][C][3][3] fp32, H and W multiples of 4 → y [N][H][W] fp32 through F(4x4,3x3) with `plane` as the contraction"""
    C, H, W = x.shape
    N = w.shape[0]
    th, tw = H // 4, W // 4
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    bt, at = BT.astype(np.float32), AT.astype(np.float32)
    d = np.stack([xp[:, 4 * i:4 * i + 6, 4 * j:4 * j + 6] for i in range(th) for j in range(tw)])      # [T][C][6][6]
    v = np.einsum("ai,tcij->tcaj", bt, d).astype(np.float32)                                            # B^T d   (small integers times fp32: fp32 sums)
    v = np.einsum("tcaj,bj->tcab", v, bt).astype(np.float32)                                            # ... B
    u = np.einsum("ai,ncij,bj->ncab", G, w.astype(np.float64), G).astype(np.float32)                    # float64, rounded once
    m = np.empty((th * tw, N, 6, 6), dtype=np.float32)
    for a in range(6):
        for b in range(6):
            m[:, :, a, b] = plane(torch.from_numpy(np.ascontiguousarray(v[:, :, a, b])), torch.from_numpy(np.ascontiguousarray(u[:, :, a, b]))).numpy()
    o = np.einsum("ai,tnij->tnaj", at, m).astype(np.float32)
    o = np.einsum("tnaj,bj->tnab", o, at).astype(np.float32)                                            # [T][N][4][4]
    return o.reshape(th, tw, N, 4, 4).transpose(2, 0, 3, 1, 4).reshape(N, H, W)


def test_split_planes_hold_the_f4x4_tolerance():
    C, H, W, N = 256, 12, 12, 64
    rng = np.random.default_rng(43)
    x = np.maximum(rng.standard_normal((C, H, W), dtype=np.float32), -0.5)
    w = rng.standard_normal((N, C, 3, 3), dtype=np.float32) / np.float32(np.sqrt(C * 9))
    ref = F.conv2d(torch.from_numpy(x).double()[None], torch.from_numpy(w).double(), None, stride=1, padding=1)[0].numpy()
    tol = 5e-5 * max(1.0, float(np.abs(ref).max()))
    err_split = float(np.abs(wino43(x, w, plane_split) - ref).max())
    err_fp32 = float(np.abs(wino43(x, w, plane_fp32) - ref).max())
    print(f"\nF(4x4), C {C}, {H} x {W}, N {N}: max |err| against float64: split planes {err_split:.3g}, fp32 planes {err_fp32:.3g} (tolerance {tol:.3g})")
    assert err_fp32 <= tol, "the emulation itself (fp32 planes) misses the tolerance"
    assert err_split <= tol, f"split planes: max abs err {err_split} > {tol}"
