"""Crown cleaning by polygon IoU (reference TreeDetection/helpers.py:602-701 ``clean_crowns`` with utilities.py:209-212
``calc_iou``; detectree2's rule): of crowns whose OUTLINES overlap at more than ``iou_threshold`` only the one with the largest
field value stays. The crown stage's own de-duplication (postprocessing.filter_polygons_by_iou_and_area, containment) works on
bounding boxes, which calls neighbours with overlapping boxes and disjoint outlines duplicates; this one does not.

What runs where: candidate pairs come from the boxes (box_pairs.candidate_pairs: the sparse pair kernels, or a host sweep); the area of
the intersection of every candidate pair is one launch of ``td_ring_pairs_area_dev`` (ringiou.hip: a wave per pair, the
fan-decomposition formula of csrc/ring_clip.h in float64) or, with ``device=None``, its host twin ``td_ring_pairs_area`` — the
two agree bit for bit; IoU is formed here and nowhere else: ``inter / ((area_a + area_b) - inter)``; the selection loop is host
Python on the sparse result. Exterior rings only (polygons with holes are not handled, as in ``process_layer``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .box_pairs import candidate_pairs, candidate_pairs_host  # noqa: F401  (re-exported)
from .crown_device import nonempty, open_ring, pack_rings, upload_rings

BELOW_ONE = float(np.nextafter(1.0, 0.0))


# ---- areas of ring pairs ------------------------------------------------------------------------------------------------------
def ring_pairs_area_packed(xy_a, start_a, xy_b, start_b, pairs, device: Optional[int] = 0, host_for_capped: bool = True):
    """td_ring_pairs_area_dev (``device``: a GPU index) or td_ring_pairs_area (``device=None``) on packed rings →
    (out float64 [k, 3] = inter, |area_a|, |area_b|; status int32 [k]). Pairs the kernel leaves to the host (status 1: more than
    ``_lib.RING_PAIR_CAP`` vertices in the two rings) are computed by the host function — same bits — unless ``host_for_capped``
    is False; the status returned is the kernel's either way. Refused pairs (status 2) are returned as NaN, not raised here."""
    same = xy_b is xy_a and start_b is start_a          # one ring set on both sides: uploaded once
    xy_a = np.ascontiguousarray(xy_a, dtype=np.float64).reshape(-1, 2)
    start_a = np.ascontiguousarray(start_a, dtype=np.int64)
    xy_b = xy_a if same else np.ascontiguousarray(xy_b, dtype=np.float64).reshape(-1, 2)
    start_b = start_a if same else np.ascontiguousarray(start_b, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    for who, xy, st in (("a", xy_a, start_a), ("b", xy_b, start_b)):
        if st.ndim != 1 or st.size < 1 or st[0] != 0 or (np.diff(st) < 0).any() or st[-1] != xy.shape[0]:
            raise ValueError(f"ring_pairs_area_packed: start_{who} must rise from 0 to the {xy.shape[0]} vertices of xy_{who}")
    k, n_a, n_b = pairs.shape[0], start_a.size - 1, start_b.size - 1
    out, status = np.full((k, 3), np.nan), np.zeros(k, np.int32)
    if k == 0:
        return out, status
    lib = _lib.load()

    def host(sel_pairs, sel_out, sel_status):
        _lib.check(lib.td_ring_pairs_area(nonempty(xy_a).ctypes.data, start_a.ctypes.data, n_a, nonempty(xy_b).ctypes.data, start_b.ctypes.data, n_b,
                                          sel_pairs.ctypes.data, sel_pairs.shape[0], sel_out.ctypes.data, sel_status.ctypes.data), "td_ring_pairs_area")

    if device is None:
        host(pairs, out, status)
        return out, status
    import torch
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_xa, d_sa = upload_rings(xy_a, start_a, dev)
        d_xb, d_sb = (d_xa, d_sa) if same else upload_rings(xy_b, start_b, dev)
        d_p = torch.from_numpy(pairs).to(dev)
        d_o = torch.empty((k, 3), dtype=torch.float64, device=dev)
        d_s = torch.empty(k, dtype=torch.int32, device=dev)
        _lib.check(lib.td_ring_pairs_area_dev(d_xa.data_ptr(), d_sa.data_ptr(), n_a, d_xb.data_ptr(), d_sb.data_ptr(), n_b, d_p.data_ptr(), k,
                                              d_o.data_ptr(), d_s.data_ptr(), _lib.stream_ptr()), "td_ring_pairs_area_dev")
        out, status = d_o.cpu().numpy(), d_s.cpu().numpy()
    capped = np.flatnonzero(status == 1)
    if capped.size and host_for_capped:
        sub_out, sub_status = np.full((capped.size, 3), np.nan), np.zeros(capped.size, np.int32)
        host(np.ascontiguousarray(pairs[capped]), sub_out, sub_status)
        out[capped] = sub_out
    return out, status


def iou_of(areas: np.ndarray) -> np.ndarray:
    """THE place IoU is formed: ``inter / ((area_a + area_b) - inter)`` on [k, 3] = inter, area_a, area_b (0 / 0 = NaN)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return areas[:, 0] / ((areas[:, 1] + areas[:, 2]) - areas[:, 0])


def ring_pairs_iou(rings_a: Sequence, rings_b: Sequence, pairs, device: Optional[int] = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Polygon IoU of ring pairs → (iou float64 [k], areas float64 [k, 3] = inter, |area_a|, |area_b|). ``pairs``: [k, 2], an
    index into ``rings_a`` and one into ``rings_b`` (the same list twice for pairs within one layer); rings are [m, 2] vertex
    arrays, closed or open, simple, either winding. ``device``: a GPU index, or None for the host function (same bits). ValueError
    for a pair the library refuses: an index outside its list, a ring of fewer than 3 vertices, a non-finite coordinate."""
    xy_a, start_a = pack_rings(rings_a)
    xy_b, start_b = (xy_a, start_a) if rings_b is rings_a else pack_rings(rings_b)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    out, status = ring_pairs_area_packed(xy_a, start_a, xy_b, start_b, pairs, device)
    bad = np.flatnonzero((status == 2) | np.isnan(out[:, 0]))
    if bad.size:
        i, j = pairs[bad[0]]
        raise ValueError(f"ring_pairs_iou: pair {int(bad[0])} = ({int(i)}, {int(j)}) is refused: an index outside its ring list, a ring "
                         f"of fewer than 3 vertices or a non-finite coordinate ({bad.size} such pairs)")
    return iou_of(out), out


# ---- clean_crowns ---------------------------------------------------------------------------------------------------------------
def _same_cycle(a: np.ndarray, b: np.ndarray) -> bool:
    """Two open rings are the same vertex cycle up to the starting vertex and the direction."""
    if a.shape != b.shape:
        return False
    m = a.shape[0]
    for k in np.flatnonzero((b[:, 0] == a[0, 0]) & (b[:, 1] == a[0, 1])):
        if np.array_equal(np.roll(b, -int(k), axis=0), a) or np.array_equal(np.roll(b[::-1], -(m - 1 - int(k)), axis=0), a):
            return True
    return False


def _shoelace(r: np.ndarray) -> float:
    r = r - r[0]                        # (map coordinates: the products would otherwise swallow the area's low digits)
    return 0.5 * float(np.dot(r[:, 0], np.roll(r[:, 1], -1)) - np.dot(np.roll(r[:, 0], -1), r[:, 1]))


def clean_crowns(rings: Sequence, field_values: Sequence, iou_threshold: float = 0.7, confidence: float = 0.2, area_threshold: float = 1,
                 device: Optional[int] = 0) -> List[int]:
    """The reference's ``clean_crowns`` (helpers.py:602-701) restated on indices → indices into ``rings`` of the crowns that stay.

    1. Rings that are empty or not valid (``td_ring_is_valid``: GEOS' rules) are dropped.
    2. Rings with ``|area| <= area_threshold`` are dropped; the survivors keep their order (the reference's re-indexed rows).
    3. For each survivor i in order the candidates are i itself, with IoU exactly 1, and every j with IoU(i, j) > ``iou_threshold``;
       the match is the candidate with the largest field value, the lowest index on ties (pandas ``nlargest(1)``, keep first).
    4. If the match's IoU with i is below 1, i yields nothing; otherwise the match is appended.
    5. IoU(i, j) is 1 for j != i only when the two rings are the same vertex cycle up to starting vertex and direction; a computed
       IoU is otherwise capped just below 1.
    6. Finally, when ``confidence > 0``, appended entries whose field value is not ``> confidence`` are dropped.
    7. The result lists indices into the INPUT, in order of appending; a twin may repeat, as the reference's output repeats it.

    ``device``: the GPU that computes the pair areas (and the candidate pairs), or None for the host functions — same areas bit
    for bit, hence the same list. ValueError for a NaN field value and for ``iou_threshold`` outside [0, 1).

    Unpinned: GEOS is not available here, so neither the noise of its overlay in a ring's IoU with itself (taken as exactly 1
    here) nor its ``intersects`` pre-filter is reproduced — the pre-filter cannot change the result, because only IoU > threshold
    >= 0 matters and disjoint rings have IoU 0. The intersection areas carry a rounding error of a few units in the last place of
    the summed triangle areas; a decision whose IoU lies within that bound of the threshold is unspecified."""
    from .validity import ring_is_valid

    n = len(rings)
    if len(field_values) != n:
        raise ValueError(f"clean_crowns: {n} rings but {len(field_values)} field values")
    field = np.array([np.nan if v is None else float(v) for v in field_values], dtype=np.float64)
    if np.isnan(field).any():
        raise ValueError("clean_crowns: a field value is NaN (or missing)")
    if not (0 <= iou_threshold < 1):
        raise ValueError(f"clean_crowns: iou_threshold must lie in [0, 1), got {iou_threshold!r}")
    survivors, opened = [], []
    for idx, ring in enumerate(rings):
        r = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        o = open_ring(r)
        if o.shape[0] < 3 or not np.isfinite(o).all():
            continue
        if not ring_is_valid(np.concatenate([o, o[:1]])):
            continue
        if not abs(_shoelace(o)) > area_threshold:
            continue
        survivors.append(idx)
        opened.append(o)
    ns = len(survivors)
    f = field[survivors] if ns else np.zeros(0)
    neighbours: Dict[int, List[Tuple[int, float]]] = {}
    if ns >= 2:
        boxes = np.array([[o[:, 0].min(), o[:, 1].min(), o[:, 0].max(), o[:, 1].max()] for o in opened])
        pairs = candidate_pairs_host(boxes) if device is None else candidate_pairs(boxes, device)
        iou, _ = ring_pairs_iou(opened, opened, pairs, device)
        for k in np.flatnonzero(iou > iou_threshold):
            i, j = int(pairs[k, 0]), int(pairs[k, 1])
            v = 1.0 if _same_cycle(opened[i], opened[j]) else min(float(iou[k]), BELOW_ONE)
            if v > iou_threshold:
                neighbours.setdefault(i, []).append((j, v))
                neighbours.setdefault(j, []).append((i, v))
    kept: List[int] = []
    for i in range(ns):
        best, best_iou = i, 1.0
        for j, v in neighbours.get(i, ()):
            if f[j] > f[best] or (f[j] == f[best] and j < best):
                best, best_iou = j, v
        if best_iou < 1.0:
            continue
        kept.append(best)
    if confidence > 0:
        kept = [k for k in kept if f[k] > confidence]
    return [survivors[k] for k in kept]


def clean_crowns_file(in_path: str, out_path: str, field: str = "Confidence_score", **kw) -> List[int]:
    """read_layer → :func:`clean_crowns` on the column ``field`` → write_blobs: the kept features, every column carried, the
    geometry blobs untouched (the way process_single_file reads and writes a layer). → the kept indices."""
    from .gpkg import read_layer, write_blobs

    layer = read_layer(in_path)
    if len(layer) and field not in layer.columns:
        raise ValueError(f"clean_crowns_file: {in_path} has no column {field!r} (it has {sorted(layer.columns)})")
    rings = layer.rings()
    kept = clean_crowns(rings, layer.columns.get(field, []), **kw)
    cols = {name: [values[i] for i in kept] for name, values in layer.columns.items()} if kept else {}
    extent = None
    if kept:
        xy = np.concatenate([rings[i] for i in kept])
        extent = (float(xy[:, 0].min()), float(xy[:, 1].min()), float(xy[:, 0].max()), float(xy[:, 1].max()))
    write_blobs(out_path, (layer.blob(i) for i in kept), cols, layer.srs_id, extent)
    return kept


def clean_crowns_setting(value=False) -> bool:
    """The ``clean_crowns`` config key: true / false (default). Anything else is refused."""
    if value is None:
        value = False
    if not any(value is v for v in (True, False)) and value not in ("true", "false"):
        raise ValueError(f"clean_crowns must be true or false, got {value!r}")
    return value in (True, "true")
