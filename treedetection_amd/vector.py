"""Polygon layers in and out of the outline steps: readers for the vector formats the reference opens with
``gpd.read_file`` (forest outline ``forrest_outline``: helpers.py:735, preprocessing.py:155; exclude files:
helpers.py:41) — GeoJSON, GeoPackage and ESRI Shapefile — and the ctypes wrapper of ``td_region_relate`` / ``td_region_relate_dev``.

A layer comes back as a list of polygons, each a list of closed rings ``[n,2] float64`` (shell first, then holes);
MultiPolygons are flattened into their parts (the predicates below work on the union anyway). No reprojection:
there is no PROJ here, so callers compare EPSG codes and refuse mixed layers instead of ``to_crs``.
"""
from __future__ import annotations

import json
import os
import re
import sqlite3
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .crown_device import decline, nonempty, take_rings

Polygon = List[np.ndarray]


# ---- WKB (ISO and EWKB flavours, both byte orders) ------------------------------------------------------
def _wkb_polygons(buf: bytes, off: int = 0) -> Tuple[List[Polygon], int]:
    order = "<" if buf[off] == 1 else ">"
    (gtype,) = struct.unpack_from(order + "I", buf, off + 1)
    off += 5
    has_z = bool(gtype & 0x80000000) or (gtype % 10000) // 1000 in (1, 3)
    has_m = bool(gtype & 0x40000000) or (gtype % 10000) // 1000 in (2, 3)
    if gtype & 0x20000000:          # EWKB SRID
        off += 4
    base = (gtype & 0x0fffffff) % 1000
    dims = 2 + has_z + has_m
    if base == 3:
        (nrings,) = struct.unpack_from(order + "I", buf, off)
        off += 4
        rings = []
        for _ in range(nrings):
            (npts,) = struct.unpack_from(order + "I", buf, off)
            off += 4
            pts = np.frombuffer(buf, dtype=order + "f8", count=npts * dims, offset=off).reshape(npts, dims)
            off += npts * dims * 8
            rings.append(np.ascontiguousarray(pts[:, :2], dtype=np.float64))
        return ([rings] if rings else []), off
    if base in (6, 7):              # MultiPolygon / GeometryCollection
        (n,) = struct.unpack_from(order + "I", buf, off)
        off += 4
        out: List[Polygon] = []
        for _ in range(n):
            part, off = _wkb_polygons(buf, off)
            out.extend(part)
        return out, off
    raise ValueError(f"WKB geometry type {gtype} is not a polygon type")


def _gpkg_geom(blob: bytes) -> List[Polygon]:
    if blob is None or len(blob) < 8 or blob[:2] != b"GP":
        return []
    flags = blob[3]
    if flags & 0x10:                # empty geometry
        return []
    env = {0: 0, 1: 32, 2: 48, 3: 48, 4: 64}[(flags >> 1) & 7]
    return _wkb_polygons(blob, 8 + env)[0]


def _read_gpkg(path: str) -> Tuple[List[Polygon], Optional[int], list]:
    con = sqlite3.connect(path)
    try:
        row = con.execute("SELECT table_name, srs_id FROM gpkg_contents WHERE data_type='features' LIMIT 1").fetchone()
        if row is None:
            return [], None, []
        table, srs_id = row
        col = con.execute("SELECT column_name FROM gpkg_geometry_columns WHERE table_name=?", (table,)).fetchone()[0]
        epsg = None
        r = con.execute("SELECT organization, organization_coordsys_id FROM gpkg_spatial_ref_sys WHERE srs_id=?", (srs_id,)).fetchone()
        if r and str(r[0]).upper() == "EPSG":
            epsg = int(r[1])
        polys, owner = [], []
        for fid, (blob,) in enumerate(con.execute(f'SELECT "{col}" FROM "{table}"')):
            parts = _gpkg_geom(blob)
            polys.extend(parts)
            owner.extend([fid] * len(parts))
        return polys, epsg, owner
    finally:
        con.close()


def _read_geojson(path: str) -> Tuple[List[Polygon], Optional[int], list]:
    with open(path) as f:
        gj = json.load(f)
    epsg = None
    name = (((gj.get("crs") or {}).get("properties") or {}).get("name")) or ""
    m = re.search(r"EPSG:+(\d+)", name.upper().replace("::", ":"))
    if m:
        epsg = int(m.group(1))      # a file without a crs member stays "unknown": it is used in the rasters' CRS as is
    polys, owner = [], []
    feats = gj.get("features", [gj] if gj.get("type") == "Feature" else [])
    for fid, feat in enumerate(feats):
        g = feat.get("geometry") or {}
        parts = []
        if g.get("type") == "Polygon":
            parts = [g["coordinates"]]
        elif g.get("type") == "MultiPolygon":
            parts = g["coordinates"]
        for part in parts:
            rings = [np.asarray(r, dtype=np.float64)[:, :2].copy() for r in part if len(r) >= 4]
            if rings:
                polys.append(rings)
                owner.append(fid)
    return polys, epsg, owner


def _ring_area2(r: np.ndarray) -> float:
    return float(np.dot(r[:-1, 0], r[1:, 1]) - np.dot(r[1:, 0], r[:-1, 1]))


def _point_in_ring(p, ring: np.ndarray) -> bool:
    x, y = ring[:-1, 0], ring[:-1, 1]
    x2, y2 = ring[1:, 0], ring[1:, 1]
    cond = (y <= p[1]) != (y2 <= p[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = x + (p[1] - y) * (x2 - x) / (y2 - y)
    return bool(np.count_nonzero(cond & (xi > p[0])) % 2)


def _read_shp(path: str) -> Tuple[List[Polygon], Optional[int], list]:
    """ESRI Shapefile main file: Polygon / PolygonZ / PolygonM records (shape types 5, 15, 25). Rings wound clockwise
    are shells, counter-clockwise rings are holes of the shell of the same record that contains them."""
    with open(path, "rb") as f:
        buf = f.read()
    if struct.unpack_from(">i", buf, 0)[0] != 9994:
        raise ValueError(f"{path}: not a shapefile")
    polys, owner = [], []
    off, fid = 100, 0
    while off + 8 <= len(buf):
        _, clen = struct.unpack_from(">ii", buf, off)
        rec = off + 8
        off = rec + 2 * clen
        (stype,) = struct.unpack_from("<i", buf, rec)
        if stype in (5, 15, 25):
            nparts, npts = struct.unpack_from("<ii", buf, rec + 36)
            parts = list(struct.unpack_from(f"<{nparts}i", buf, rec + 44)) + [npts]
            pts = np.frombuffer(buf, dtype="<f8", count=2 * npts, offset=rec + 44 + 4 * nparts).reshape(npts, 2)
            shells, holes = [], []
            for a, b in zip(parts[:-1], parts[1:]):
                ring = np.array(pts[a:b], dtype=np.float64)
                if len(ring) < 4:
                    continue
                (shells if _ring_area2(ring) < 0 else holes).append(ring)
            if not shells and holes:            # writers that ignore the winding rule: treat the rings as shells
                shells, holes = holes, []
            rec_polys = [[s] for s in shells]
            for h in holes:
                for poly in rec_polys:
                    if _point_in_ring(h[0], poly[0]):
                        poly.append(h)
                        break
            polys.extend(rec_polys)
            owner.extend([fid] * len(rec_polys))
        fid += 1
    epsg = None
    prj = os.path.splitext(path)[0] + ".prj"
    if os.path.exists(prj):
        with open(prj) as f:
            m = re.findall(r'AUTHORITY\["EPSG","(\d+)"\]', f.read())
        if m:
            epsg = int(m[-1])
    return polys, epsg, owner


def read_polygon_layer(path: str, with_owner: bool = False):
    """→ (polygons, epsg or None) — or (polygons, epsg, feature index per polygon) with ``with_owner``."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".gpkg":
        polys, epsg, owner = _read_gpkg(path)
    elif ext in (".geojson", ".json"):
        polys, epsg, owner = _read_geojson(path)
    elif ext == ".shp":
        polys, epsg, owner = _read_shp(path)
    else:
        raise ValueError(f"{path}: unsupported vector format (GeoJSON, GeoPackage and Shapefile are read)")
    for poly in polys:
        for i, r in enumerate(poly):
            if not (r[0] == r[-1]).all():
                poly[i] = np.concatenate([r, r[:1]])
    return (polys, epsg, owner) if with_owner else (polys, epsg)


# ---- predicates ------------------------------------------------------------------------------------------
class Region:
    """Polygons with holes, packed once for ``td_region_relate``."""

    def __init__(self, polygons: Sequence[Polygon]):
        rings = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 2) for poly in polygons for r in poly]
        self.ring_poly = np.asarray([i for i, poly in enumerate(polygons) for _ in poly], dtype=np.int32)
        self.ring_start = np.zeros(len(rings) + 1, dtype=np.int64)
        if rings:
            self.ring_start[1:] = np.cumsum([len(r) for r in rings])
        self.xy = np.concatenate(rings) if rings else np.zeros((0, 2))
        self.n_rings = len(rings)
        if rings:
            self.bounds = (float(self.xy[:, 0].min()), float(self.xy[:, 1].min()), float(self.xy[:, 0].max()), float(self.xy[:, 1].max()))
        else:
            self.bounds = None
        self.last_deferred = 0          # queries of the last relate(device=...) that the kernel left to the host function,
        self.last_deferred_queries = np.zeros(0, dtype=np.int64)          # and which
        self._index = None              # build_edge_index of this region (False: it does not fit int32), built on first device use
        self._on_device = {}            # GPU index → the region and its index as uploaded tensors

    def relate(self, queries: Sequence[np.ndarray], device: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """closed query rings → (intersects[n], within[n]) against the union of the polygons.

        ``device=None``: ``td_region_relate`` on the host. ``device`` = a GPU index: ``td_region_relate_dev`` (regionrelate.hip, a wave
        per query, the host function's arithmetic) — the region and its y-bin edge index are packed and uploaded once per Region and
        device and kept on the object, the queries are packed and uploaded, ONE launch on the current stream decides them, flags and
        status come back, and the queries the kernel left undecided (status 1: a ring or a run of meetings beyond its fixed
        capacities, ``_lib.RELATE_*_CAP``) — only those — go through the host function; ``last_deferred`` says how many that were.
        Same flags either way. Rings the host call refuses (not closed, fewer than 4 points) raise what it raises, before any launch.
        A set the device path does not take (an empty region, a non-finite coordinate, more edges, index entries or queries than
        int32 holds) is announced in one printed line and served by the host function."""
        n = len(queries)
        flags = np.zeros(n, dtype=np.uint8)
        self.last_deferred, self.last_deferred_queries = 0, np.zeros(0, dtype=np.int64)
        if n == 0 or self.n_rings == 0:
            if device is not None and n:
                decline("Region.relate", "the region is empty")
            return flags.astype(bool), flags.astype(bool)
        qs = [np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 2) for q in queries]
        q_start = np.zeros(n + 1, dtype=np.int64)
        q_start[1:] = np.cumsum([len(q) for q in qs])
        q_xy = np.concatenate(qs)
        if device is not None and self._rings_refused(self.xy, self.ring_start) is None and self._rings_refused(q_xy, q_start) is None:
            why = self._device_declined(q_xy, n)
            if why is None:
                flags = self._relate_device(q_xy, q_start, n, int(device))
                return (flags & 1).astype(bool), (flags & 2).astype(bool)
            decline("Region.relate", why)
        # (a ring the library refuses reaches it here, device or not, and raises there)
        self._relate_host(q_xy, q_start, n, flags)
        return (flags & 1).astype(bool), (flags & 2).astype(bool)

    def _relate_host(self, q_xy, q_start, n, flags) -> None:
        st = _lib.load().td_region_relate(self.xy.ctypes.data, self.ring_start.ctypes.data, self.ring_poly.ctypes.data,
                                          self.n_rings, q_xy.ctypes.data, q_start.ctypes.data, n, flags.ctypes.data)
        _lib.check(st, "td_region_relate")

    @staticmethod
    def _rings_refused(xy: np.ndarray, start: np.ndarray) -> Optional[int]:
        """Index of the first ring td_region_relate refuses (fewer than 4 points, first != last — a NaN there included), or None."""
        first, last = xy[start[:-1].clip(max=len(xy) - 1)], xy[(start[1:] - 1).clip(min=0)]
        bad = (np.diff(start) < 4) | ~((first == last).all(axis=1))
        return int(np.argmax(bad)) if bad.any() else None

    def _device_declined(self, q_xy: np.ndarray, n: int) -> Optional[str]:
        """Why td_region_relate_dev must not see this region / these queries, or None."""
        if not (np.isfinite(self.xy).all() and np.isfinite(q_xy).all()):
            return "a coordinate is not finite"
        if len(self.xy) >= INT32_LIMIT or n >= INT32_LIMIT:
            return f"more than {INT32_LIMIT - 1} region vertices or queries"
        if self._index is None:
            self._index = build_edge_index(self.xy, self.ring_start)
        if self._index is False:
            return f"more than {INT32_LIMIT - 1} entries in the edge index"
        return None

    def _relate_device(self, q_xy, q_start, n, device: int) -> np.ndarray:
        import torch
        lib = _lib.load()
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(a).to(dev)
            R = self._on_device.get(device)
            if R is None:
                edge_ring, bin_start, bin_edges = self._index[:3]
                R = self._on_device[device] = {"xy": up(self.xy), "ring_start": up(self.ring_start), "ring_poly": up(self.ring_poly),
                                               "edge_ring": up(edge_ring), "bin_start": up(bin_start),
                                               "bin_edges": up(nonempty(bin_edges)),
                                               "n_bin_edges": int(bin_edges.size), "checked": False}
            ymin, ymax, inv_h = self._index[3:]
            d_q, d_qs = up(q_xy), up(q_start)
            d_f = torch.empty(n, dtype=torch.uint8, device=dev)
            d_s = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(lib.td_region_relate_dev(R["xy"].data_ptr(), R["ring_start"].data_ptr(), R["ring_poly"].data_ptr(), self.n_rings,
                                                len(self.xy), R["edge_ring"].data_ptr(), R["bin_start"].data_ptr(), R["bin_edges"].data_ptr(),
                                                len(R["bin_start"]) - 1, R["n_bin_edges"], ymin, ymax, inv_h, d_q.data_ptr(), d_qs.data_ptr(),
                                                n, len(q_xy), d_f.data_ptr(), d_s.data_ptr(), 0 if R["checked"] else 1, _lib.stream_ptr()),
                       "td_region_relate_dev")
            R["checked"] = True             # the uploaded index was verified against its arrays by that call
            flags, status = d_f.cpu().numpy(), d_s.cpu().numpy()
        if (status == 2).any():             # cannot happen after _rings_refused / _device_declined
            raise _lib.TdError(f"td_region_relate_dev refused query {int(np.argmax(status == 2))}")
        deferred = np.flatnonzero(status == 1)
        self.last_deferred, self.last_deferred_queries = int(deferred.size), deferred
        if deferred.size:
            sub_flags = np.zeros(deferred.size, dtype=np.uint8)
            self._relate_host(*take_rings(q_xy, q_start, deferred), int(deferred.size), sub_flags)
            flags[deferred] = sub_flags
        return flags


INT32_LIMIT = 2 ** 31 - 1


def build_edge_index(xy: np.ndarray, ring_start: np.ndarray):
    """The y-bin edge index of ``td_region_relate`` (csrc/region.cpp: same bin count, same bin of a y) as the flat arrays
    ``td_region_relate_dev`` takes → (edge_ring int32 [n_vertices], bin_start int32 [n_bins + 1], bin_edges int32, ymin, ymax, inv_h),
    or False when the entries do not fit int32. Edge id = index of the edge's first vertex; an edge is listed in every bin its
    y-range touches; the ids of a bin ascend. ``xy``: finite closed rings of >= 4 points."""
    n_rings = len(ring_start) - 1
    edge_ring = np.repeat(np.arange(n_rings, dtype=np.int32), np.diff(ring_start))
    is_edge = np.ones(len(xy), dtype=bool)
    is_edge[ring_start[1:] - 1] = False                  # a ring's closing vertex starts no edge
    ids = np.flatnonzero(is_edge)
    y = xy[:, 1]
    ymin, ymax = float(y.min()), float(y.max())
    nb = int(min(8192, max(1, len(ids) // 4)))
    inv_h = nb / (ymax - ymin) if ymax > ymin else 0.0

    def bin_of(v):
        f = (v - ymin) * inv_h
        with np.errstate(invalid="ignore"):
            return np.where(f > 0, np.where(f >= nb, nb - 1, np.floor(np.minimum(f, nb))), 0).astype(np.int64)

    b0, b1 = bin_of(np.fmin(y[ids], y[ids + 1])), bin_of(np.fmax(y[ids], y[ids + 1]))
    count = b1 - b0 + 1
    total = int(count.sum())
    if total >= INT32_LIMIT:
        return False
    first = np.cumsum(count) - count
    bins = np.repeat(b0 - first, count) + np.arange(total)
    order = np.argsort(bins, kind="stable")              # ids stay ascending inside a bin
    bin_edges = np.repeat(ids, count)[order].astype(np.int32)
    bin_start = np.zeros(nb + 1, dtype=np.int32)
    bin_start[1:] = np.cumsum(np.bincount(bins, minlength=nb))
    return edge_ring, bin_start, bin_edges, ymin, ymax, float(inv_h)


def box_ring(minx, miny, maxx, maxy) -> np.ndarray:
    """shapely.geometry.box's ring (counter-clockwise from the lower right corner)."""
    return np.array([[maxx, miny], [maxx, maxy], [minx, maxy], [minx, miny], [maxx, miny]], dtype=np.float64)
