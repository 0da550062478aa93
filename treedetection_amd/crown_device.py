"""The base layer of the crown stage's device wrappers: what box_pairs, crown_rasters, cleaning, evaluation and vector share around a
kernel and its host twin. No sibling is imported, and torch only inside the functions that upload: ``device=None`` never loads it.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np


def decline(who: str, why: str) -> None:
    """The one line a device path prints when it leaves its input to the host function."""
    print(f"{who}: {why}: using the host function")


def nonempty(a: np.ndarray) -> np.ndarray:
    """``a`` itself, or for an empty array one zero row of its dtype: an empty array still needs a pointer the library accepts."""
    return a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)


def open_ring(ring) -> np.ndarray:
    """[m, 2] float64 without the repeated closing vertex (a closed ring, as Layer.rings() gives it, loses its last vertex)."""
    r = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    if r.shape[0] >= 2 and r[0, 0] == r[-1, 0] and r[0, 1] == r[-1, 1]:
        r = r[:-1]
    return r


def pack_rings(rings: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """Open rings concatenated for td_ring_pairs_area: (xy float64 [total, 2], start int64 [n + 1])."""
    opened = [open_ring(r) for r in rings]
    start = np.zeros(len(opened) + 1, np.int64)
    if opened:
        np.cumsum([r.shape[0] for r in opened], out=start[1:])
    xy = np.concatenate(opened) if opened and start[-1] else np.zeros((0, 2))
    return np.ascontiguousarray(xy, dtype=np.float64), start


def take_rings(xy: np.ndarray, start: np.ndarray, idx) -> Tuple[np.ndarray, np.ndarray]:
    """The rings ``idx`` (any order, repeats allowed) of a packed set as a packed set of their own, vertices untouched:
    (sub_xy float64 [total, 2], sub_start int64 [len(idx) + 1]) — what the host function gets for the rings a kernel left to it."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    lens = start[idx + 1] - start[idx]
    sub_start = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens, dtype=np.int64)])
    src = np.repeat(start[idx] - sub_start[:-1], lens) + np.arange(sub_start[-1])
    return np.ascontiguousarray(xy[src], dtype=np.float64).reshape(-1, 2), sub_start


def packed_boxes(xy: np.ndarray, start: np.ndarray) -> np.ndarray:
    """float64 [n, 4] (x1, y1, x2, y2) of rings packed as :func:`pack_rings` packs them; a ring without vertices gets a NaN box
    (it pairs with nothing), and so does a ring with a NaN coordinate."""
    n = start.size - 1
    out = np.full((n, 4), np.nan)
    full = np.flatnonzero(np.diff(start) > 0)
    if full.size:                                   # (reduceat over the non-empty rings: their segments follow one another in xy)
        out[full, :2] = np.minimum.reduceat(xy, start[full], axis=0)
        out[full, 2:] = np.maximum.reduceat(xy, start[full], axis=0)
    return out


def ring_boxes(rings: Sequence) -> np.ndarray:
    """:func:`packed_boxes` of a list of rings (closed or open)."""
    return packed_boxes(*pack_rings(rings))


def upload_rings(xy: np.ndarray, start: np.ndarray, dev):
    """Packed rings (:func:`pack_rings`) as the two device tensors td_crown_zonal_dev reads: upload once, pass to every launch."""
    import torch
    return torch.from_numpy(nonempty(xy)).to(dev), torch.from_numpy(start).to(dev)


def check_raster_tensor(raster, who: str) -> None:
    """Refuses (ValueError, in ``who``'s name) a raster given as a tensor that the kernels cannot read where it lies."""
    import torch
    if isinstance(raster, torch.Tensor) and not (raster.is_cuda and raster.dtype == torch.float32 and raster.dim() == 2 and raster.is_contiguous()):
        raise ValueError(f"{who}: a raster tensor must be a contiguous float32 CUDA tensor [rows, cols], got {raster.dtype} "
                         f"{tuple(raster.shape)} on {raster.device}")


def sparse_rows(n_rows: int, count, fill, cap: int, dev) -> Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """The two-pass store of a sparse pair kernel on the current device ``dev``: ``count(counts)`` launches the pass that writes int32
    ``counts[n_rows]``, a prefix sum gives int64 ``row_start``, ``fill(row_start, cursor, cols)`` launches the pass that stores row i in
    ``cols[row_start[i]:row_start[i + 1]]`` (not for a total of 0) → (row_start, counts, cols) on the host; None above ``cap`` pairs."""
    import torch
    counts = torch.empty(n_rows, dtype=torch.int32, device=dev)
    count(counts)
    row_start = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=row_start[1:])
    total = int(row_start[-1].item())
    if total > cap:
        return None
    cols = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        fill(row_start, torch.empty(n_rows, dtype=torch.int32, device=dev), cols)
    row_start = row_start.cpu().numpy()
    return row_start, np.diff(row_start), cols[:total].cpu().numpy()
