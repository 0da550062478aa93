"""Crafted instance masks for the device contour tracer (treedetection_amd/csrc/contours_dev.hip, td_trace_contours_dev) at
its size, word, window and count limits, each with the status it must get, and ONE strict checker of the tracer's four
output arrays.

A case is ``Case(name, mask bool[h, w], status, why)``; ``status`` is written down here by intent (0 traced; 1 region
larger than the on-chip label image; 2 more than TD_CONTOUR_MAX contours) and tests/test_contour_cases.py proves it on the
CPU from the region size and the oracle's contour count, together with the sizes, counts and depths the names promise.
tests/test_contours_limits_gpu.py feeds the cases to the kernel.

``check_outputs`` judges a complete result (points, image_points, det_info, contour_info, all pre-filled with canaries)
against oracle/contours_ref.py; ``expected_outputs`` builds a correct result on the CPU in the device's format, which
the CPU controls perturb to show that the checker rejects each kind of damage. Nothing here needs a GPU or the library.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from oracle.contours_ref import find_contours as oracle_find_contours

CMAX = 256                  # TD_CONTOUR_MAX
LABEL_SMALL = 6 * 1024      # (w + 2) * (h + 2) int16 labels of the first launch
LABEL_LARGE = 28 * 1024     # ... of the second; larger regions get status 1
PTS_CANARY = 0x5A5A
INFO_CANARY = -7


class Case(NamedTuple):
    name: str
    mask: np.ndarray
    status: int
    why: str
    dx1: int = 0            # added to the region's x1 only (a region of negative width over a zero-width mask)


class Det(NamedTuple):
    x0: int
    y0: int
    mask: np.ndarray
    status: int
    dx1: int = 0


def need(mask: np.ndarray) -> int:
    h, w = mask.shape
    return (w + 2) * (h + 2)


def status_rule(label_elems: int, contours: int) -> int:
    """include/treedet.h: 1 region larger than the on-chip label image; 2 more than TD_CONTOUR_MAX contours; else traced."""
    return 1 if label_elems > LABEL_LARGE else 2 if contours > CMAX else 0


_ORACLE: Dict[Tuple[Tuple[int, int], bytes], List[np.ndarray]] = {}


def contours_of(mask: np.ndarray) -> List[np.ndarray]:
    """The oracle's contours of a mask, computed once per distinct mask."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    key = (m.shape, m.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = oracle_find_contours(m) if m.size else []
    return _ORACLE[key]


# ---- tree depth from the RETR_TREE order ---------------------------------------------------------------------------------
def _on_ring(p, ring) -> bool:
    px, py = int(p[0]), int(p[1])
    n = len(ring)
    for i in range(n):
        ax, ay = int(ring[i][0]), int(ring[i][1])
        bx, by = int(ring[(i + 1) % n][0]), int(ring[(i + 1) % n][1])
        if (bx - ax) * (py - ay) - (by - ay) * (px - ax) == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return True
    return False


def _inside_ring(p, ring) -> bool:
    """Even-odd rule on the closed ring, integer arithmetic; only meaningful for points not on the ring."""
    px, py = int(p[0]), int(p[1])
    n, odd = len(ring), False
    for i in range(n):
        ax, ay = int(ring[i][0]), int(ring[i][1])
        bx, by = int(ring[(i + 1) % n][0]), int(ring[(i + 1) % n][1])
        if (ay > py) != (by > py):
            # x of the edge at height py, compared with px without dividing
            lhs, rhs = (px - ax) * (by - ay), (bx - ax) * (py - ay)
            if (lhs < rhs) == (by > ay):
                odd = not odd
    return odd


def tree_depths(contours: Sequence[np.ndarray]) -> List[int]:
    """Depth of every contour (0 = top level) from the pre-order list alone, by containment of the contour's first point in the
    rings before it. Top-level contours are outer borders and the levels alternate. A hole border runs on pixels of its own
    component, so its first point may lie ON the outer border that encloses it: under an outer border the test is inclusive.
    An outer border inside a hole is a different component, at least two pixels from the hole border's pixels: under a hole
    border the test is strict, which also keeps a hole from passing as the child of a sibling hole it shares pixels with."""
    stack: List[int] = []
    depth = []
    for i, c in enumerate(contours):
        p = c[0]
        while stack:
            t = contours[stack[-1]]
            outer = len(stack) % 2 == 1
            on = _on_ring(p, t)
            if (on and outer) or (not on and _inside_ring(p, t)):
                break
            stack.pop()
        depth.append(len(stack))
        stack.append(i)
    return depth


# ---- the families ----------------------------------------------------------------------------------------------------------
def _blob_with_hole(h: int, w: int) -> np.ndarray:
    """The ellipse inscribed in the region (touches all four edges) minus a concentric ellipse of a third of its axes. At
    w == 1 that is a column cut in two, at w == 3 a column with a long one-pixel hole."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    m = ((xx - cx) / (w / 2.0)) ** 2 + ((yy - cy) / (h / 2.0)) ** 2 <= 1.0
    m &= ~(((xx - cx) / (w / 6.0)) ** 2 + ((yy - cy) / (h / 6.0)) ** 2 < 1.0)
    return m


# (label elements, w, h, expected status): the table of the size classes
SIZE_TABLE = [(6144, 94, 62, 0), (6144, 62, 94, 0), (6150, 73, 80, 0), (6147, 1, 2047, 0), (6145, 3, 1227, 0), (28672, 126, 222, 0),
              (28673, 51, 539, 1), (28836, 176, 160, 1)]


def size_cases() -> List[Case]:
    out = []
    for elems, w, h, st in SIZE_TABLE:
        cls = "small class" if elems <= LABEL_SMALL else "large class" if elems <= LABEL_LARGE else "too large"
        out.append(Case(f"blob-{w}x{h}", _blob_with_hole(h, w), st, f"{elems} label elements: {cls}"))
    out.append(Case("ones-94x62", np.ones((62, 94), bool), 0, "all ones, last of the small class: one contour of four points"))
    out.append(Case("ones-126x222", np.ones((222, 126), bool), 0, "all ones, last of the large class: one contour of four points"))
    return out


WORD_WIDTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129)
BAR_ENDS = (31, 32, 33, 63, 64, 65)         # last column of the left bar; the gap is the column after it
BAR_ENDS_APART = (31, 63, 64)


def _comb(w: int) -> np.ndarray:
    m = np.zeros((5, w), bool)
    m[0, :] = True
    for t in (5, 20, 41, 63):
        m[1:, t] = True
    for r, c in ((2, 10), (2, 30), (2, 50), (4, 7), (4, 39), (4, 61)):
        m[r, c] = True
    return m


# name -> (width, rung columns, columns of the isolated pixels in row 2)
LADDERS = {"w64-ladder": (64, (0, 5, 20, 41, 63), (2, 7, 18, 30, 43, 61)),
           "w65-ladder": (65, (0, 5, 20, 41, 64), (2, 7, 18, 30, 43, 62)),
           # row 2 has no candidate in its first window, only the marks of four rungs; the pixel is lane 0 of the second window
           "w129-ladder-60": (129, (0, 20, 40, 60, 100, 105, 128), (64, 110)),
           # ... the last of those marks is lane 63, the pixel lane 1 of the second window
           "w129-ladder-63": (129, (0, 20, 40, 63, 100, 105, 128), (65, 110))}


def _ladder(w: int, rungs, pixels) -> np.ndarray:
    m = np.zeros((5, w), bool)
    m[0, :] = m[4, :] = True
    for t in rungs:
        m[1:4, t] = True
    for c in pixels:
        m[2, c] = True
    return m


def word_cases() -> List[Case]:
    out = []
    for w in WORD_WIDTHS:
        m = np.ones((5, w), bool)
        out.append(Case(f"w{w}-ones", m, 0, "all ones: the right edge is the last bit of a word / the last lane of a window"))
        m = np.zeros((5, w), bool)
        m[2, w - 1] = True
        out.append(Case(f"w{w}-last", m, 0, "one pixel in the last column: an outer start there"))
        m = np.zeros((5, w), bool)
        m[2, 0] = True
        out.append(Case(f"w{w}-first", m, 0, "one pixel in the first column"))
        m = np.zeros((5, w), bool)
        m[:, ::2] = True
        out.append(Case(f"w{w}-stripes", m, 0, "1-px stripes of period 2: every window restarts one past a candidate"))
        for a in BAR_ENDS:
            if w < a + 3:
                continue
            if a in BAR_ENDS_APART:
                m = np.ones((5, w), bool)
                m[:, a + 1] = False
                out.append(Case(f"w{w}-bars-{a}|{a + 1}", m, 0, f"two solid bars, gap at column {a + 1}: the second bar starts at {a + 2}"))
            m = np.ones((5, w), bool)
            m[1:4, a + 1] = False
            out.append(Case(f"w{w}-bridge-{a}|{a + 1}", m, 0, f"bars joined above and below the gap: a hole start at column {a}, its zero neighbour at {a + 1}"))
    for w in (64, 65):
        out.append(Case(f"w{w}-comb", _comb(w), 0, "one outer contour along row 0; rows 1-4 meet its marked teeth before, between and after candidates"))
        out.append(Case(f"w{w}-ladder", _ladder(*LADDERS[f"w{w}-ladder"]), 0, "a comb closed below: the pixel in each cell hangs under the hole whose mark precedes it"))
    for a in (60, 63):
        out.append(Case(f"w129-ladder-{a}", _ladder(*LADDERS[f"w129-ladder-{a}"]), 0,
                        f"a window of marks only, the last at column {a}, decides the parent of the first pixel of the next window; two marks precede the second pixel"))
    m = np.zeros((9, 130), bool)
    m[0, :] = m[8, :] = True
    m[:, 0] = m[:, 129] = True
    m[2, 65:71] = m[6, 65:71] = True
    m[2:7, 65] = m[2:7, 70] = True
    out.append(Case("w130-rings", m, 0, "a 1-px frame with a second ring whose left edge is column 65: outer and hole start in the second window"))
    return out


def _isolated(n: int, w: int = 63, extra_rows: int = 0) -> np.ndarray:
    per_row = (w + 1) // 2
    rows = (n + per_row - 1) // per_row
    m = np.zeros((2 * rows - 1 + extra_rows, w), bool)
    for i in range(n):
        m[2 * (i // per_row), 2 * (i % per_row)] = True
    return m


def _rings128(w: int = 63, h: int = 31) -> np.ndarray:
    m = np.zeros((h, w), bool)
    for i in range(128):
        r, c = 4 * (i // 16), 4 * (i % 16)
        m[r:r + 3, c:c + 3] = True
        m[r + 1, c + 1] = False
    return m


def count_cases() -> List[Case]:
    out = [Case("iso-256", _isolated(256), 0, "exactly TD_CONTOUR_MAX contours"),
           Case("iso-257", _isolated(257), 2, "one contour too many"),
           Case("rings-128", _rings128(), 0, "128 outer + 128 hole borders = TD_CONTOUR_MAX, outer and hole labels interleaved")]
    m = _rings128(w=65)
    m[0, 64] = True
    out.append(Case("rings-128-plus-1", m, 2, "a 17th border in row 0: the limit trips at the last ring's hole"))
    out.append(Case("iso-65", _isolated(65), 0, "the re-trace loop takes two rounds"))
    out.append(Case("iso-129", _isolated(129), 0, "the re-trace loop takes three rounds"))
    m = _isolated(256, extra_rows=4)
    m[-1, -1] = True
    out.append(Case("iso-256-late-257th", m, 2, "the 257th start is the last pixel of the last row, after 256 borders were followed"))
    return out


def _square_rings(depth: int) -> np.ndarray:
    n = 4 * depth + 1
    m = np.zeros((n, n), bool)
    for k in range(depth):
        a, b = 2 * k, n - 1 - 2 * k
        m[a, a:b + 1] = m[b, a:b + 1] = True
        m[a:b + 1, a] = m[a:b + 1, b] = True
    m[n // 2, n // 2] = True
    return m


def nest_cases() -> List[Case]:
    out = [Case("rings-18", _square_rings(18), 0, "18 concentric rings and a centre pixel: 37 levels, small class"),
           Case("rings-30", _square_rings(30), 0, "30 concentric rings and a centre pixel: 61 levels, large class")]
    s = _square_rings(4)                                  # 17 x 17
    m = np.zeros((21, 39), bool)
    m[0, :] = m[20, :] = True
    m[:, 0] = m[:, 38] = True
    m[2:19, 2:19] = s
    m[2:19, 20:37] = s
    out.append(Case("twin-stacks", m, 0, "two stacks of 4 rings side by side inside one ring: siblings at every level"))
    m = np.zeros((14, 24), bool)
    m[0, :] = m[13, :] = True
    m[:, 0] = m[:, 23] = True
    for r0, r1, c0, c1 in ((2, 5, 2, 5), (3, 8, 8, 12), (6, 12, 15, 21)):      # a 3x3, a 5x4 and a 6x6 ring
        m[r0:r1, c0:c1] = True
        m[r0 + 1:r1 - 1, c0 + 1:c1 - 1] = False
    out.append(Case("three-islands", m, 0, "a hole with three islands, each with its own hole: sibling order under a hole"))
    m = np.zeros((20, 20), bool)
    m[np.arange(20), np.arange(20)] = True
    out.append(Case("diagonal-line", m, 0, "pixels touching only at corners: the outer border passes every inner pixel twice"))
    m = np.zeros((16, 16), bool)
    for i in range(8):
        m[2 * i:2 * i + 2, 2 * i:2 * i + 2] = True
    out.append(Case("staircase", m, 0, "2x2 blocks touching at corners: one 8-connected outer border"))
    yy, xx = np.mgrid[0:13, 0:13]
    dist = np.abs(xx - 6) + np.abs(yy - 6)
    out.append(Case("diamond", (dist <= 6) & (dist % 2 == 0), 0, "checkerboard diamond: one outer border, 36 one-pixel holes that are 4-connected"))
    return out


def degenerate_cases() -> List[Case]:
    return [Case("1x1", np.ones((1, 1), bool), 0, "a single pixel region"),
            Case("row-70", np.ones((1, 70), bool), 0, "one row across two windows"),
            Case("column-70", np.ones((70, 1), bool), 0, "one column"),
            Case("empty-4x4", np.zeros((4, 4), bool), 0, "no contour: no point block is allocated"),
            Case("empty-5x130", np.zeros((5, 130), bool), 0, "no contour over three windows"),
            Case("zero-width", np.zeros((4, 0), bool), 0, "w == 0: four zeros"),
            Case("negative-width", np.zeros((4, 0), bool), 0, "w < 0: four zeros", dx1=-3),
            Case("zero-height", np.zeros((0, 4), bool), 0, "h == 0: four zeros")]


FAMILIES = {"size": size_cases, "word": word_cases, "count": count_cases, "nest": nest_cases, "degenerate": degenerate_cases}
_CASES: Dict[str, List[Case]] = {}


def family(name: str) -> List[Case]:
    if name not in _CASES:
        _CASES[name] = FAMILIES[name]()
    return _CASES[name]


def case(name: str) -> Case:
    for f in FAMILIES:
        for c in family(f):
            if c.name == name:
                return c
    raise KeyError(name)


def dets_of(cases: Sequence[Case], seed: int = 0) -> List[Det]:
    """The cases as detections at varied tile positions (x0 + w stays far inside int16)."""
    rng = np.random.default_rng(seed)
    return [Det(int(rng.integers(0, 1200)), int(rng.integers(0, 1200)), c.mask, c.status, c.dx1) for c in cases]


# ---- the tracer's inputs and outputs -----------------------------------------------------------------------------------------
def pack(images: Sequence[Sequence[Det]], Dn: int):
    """→ region int32 [B, Dn, 4], offset int64 [B, Dn], bits uint32 [B, words] like the paste kernel leaves them. Every entry
    is packed, also those a test puts behind the image's count; the words behind the last region hold garbage."""
    B = len(images)
    region = np.zeros((B, Dn, 4), np.int32)
    offset = np.zeros((B, Dn), np.int64)
    words = []
    for b, dets in enumerate(images):
        assert len(dets) <= Dn
        cur, off = [], 0
        for d, det in enumerate(dets):
            h, w = det.mask.shape
            wpr = (w + 31) // 32
            pad = np.zeros((h, wpr * 32), np.uint8)
            pad[:, :w] = det.mask
            rows = np.packbits(pad, axis=1, bitorder="little").view(np.uint32).ravel() if h * wpr else np.zeros(0, np.uint32)
            region[b, d] = (det.x0, det.y0, det.x0 + w + det.dx1, det.y0 + h)
            offset[b, d] = off
            off += rows.size
            cur.append(rows)
        words.append(np.concatenate(cur) if cur else np.zeros(0, np.uint32))
    wpi = max(len(x) for x in words) + 8
    bits = np.full((B, wpi), 0xA5A5A5A5, np.uint32)
    for b, x in enumerate(words):
        bits[b, : len(x)] = x
    return region, offset, bits


def canary_outputs(B: int, Dn: int, pts_cap: int) -> Dict[str, np.ndarray]:
    return {"pts": np.full((B, pts_cap, 2), PTS_CANARY, np.int16), "img_pts": np.full((B,), INFO_CANARY, np.int32),
            "det_info": np.full((B, Dn, 4), INFO_CANARY, np.int32), "cont_info": np.full((B, Dn, CMAX, 2), INFO_CANARY, np.int32)}


def _void(det: Det) -> bool:
    h, w = det.mask.shape
    return w + det.dx1 <= 0 or h <= 0


def expected_outputs(images: Sequence[Sequence[Det]], counts: Sequence[int], Dn: int, pts_cap: int) -> Dict[str, np.ndarray]:
    """A correct result in the device's format, built from the oracle: point blocks handed out in detection order (the
    device hands them out in the order its atomics land, which the checker does not prescribe)."""
    out = canary_outputs(len(images), Dn, pts_cap)
    for b, dets in enumerate(images):
        cursor = 0
        out["det_info"][b] = 0
        for d, det in enumerate(dets[: counts[b]]):
            if det.status != 0:
                out["det_info"][b, d] = (det.status, 0, 0, 0)
                continue
            cs = [] if _void(det) else contours_of(det.mask)
            total = sum(len(c) for c in cs)
            base = cursor if total else 0
            cursor += total
            if base + total > pts_cap:
                out["det_info"][b, d] = (4, 0, base, 0)
                continue
            out["det_info"][b, d] = (0, len(cs), base, total)
            o = 0
            for k, c in enumerate(cs):
                out["cont_info"][b, d, k] = (o, len(c))
                out["pts"][b, base + o: base + o + len(c)] = c + [det.x0, det.y0]
                o += len(c)
        out["img_pts"][b] = cursor
    return out


def check_outputs(out: Dict[str, np.ndarray], images: Sequence[Sequence[Det]], counts: Sequence[int], pts_cap: int,
                  full: Optional[Dict[int, int]] = None) -> Dict[int, int]:
    """Assert that ``out`` (arrays that held canaries before the launch) is exactly what the tracer must leave for the
    detections ``images[b][:counts[b]]``. ``full[b]`` = how many detections of image b the test has arranged to find the
    point buffer full (status 4); anywhere else a status 4 fails. → number of detections per status."""
    pts, img_pts, det_info, cont_info = out["pts"], out["img_pts"], out["det_info"], out["cont_info"]
    B, Dn = det_info.shape[:2]
    full = full or {}
    assert pts.shape == (B, pts_cap, 2) and cont_info.shape == (B, Dn, CMAX, 2) and len(images) == B and len(counts) == B
    seen = {0: 0, 1: 0, 2: 0, 4: 0}
    for b in range(B):
        n = int(counts[b])
        assert (det_info[b, n:] == 0).all(), f"image {b}: det_info rows at or past the count {n} are not four zeros:\n{det_info[b, n:]}"
        assert (cont_info[b, n:] == INFO_CANARY).all(), f"image {b}: cont_info written behind the count"
        spans, written, n_full = [], np.zeros(pts_cap, bool), 0
        for d in range(n):
            det = images[b][d]
            row = det_info[b, d].tolist()
            where = f"image {b} detection {d} ({det.mask.shape[1]}x{det.mask.shape[0]}): det_info {row}"
            assert INFO_CANARY not in row, f"{where}: row not written by either launch"
            status = row[0]
            if det.status != 0:
                assert row == [det.status, 0, 0, 0], f"{where}, expected status {det.status}"
                assert (cont_info[b, d] == INFO_CANARY).all(), f"{where}: a flagged detection wrote cont_info"
                seen[status] += 1
                continue
            cs = [] if _void(det) else contours_of(det.mask)
            total = sum(len(c) for c in cs)
            if status == 4:
                n_full += 1
                base = row[2]
                assert row == [4, 0, base, 0] and base >= 0 and base + total > pts_cap, f"{where}: status 4 but {base} + {total} fits {pts_cap}"
                assert (cont_info[b, d] == INFO_CANARY).all(), f"{where}: a flagged detection wrote cont_info"
                spans.append((base, total, d))
                seen[4] += 1
                continue
            assert status == 0, f"{where}, expected status 0"
            seen[0] += 1
            base = row[2]
            assert row == [0, len(cs), base, total], f"{where}, expected [0, {len(cs)}, base, {total}]"
            assert 0 <= base and base + total <= pts_cap and (total > 0 or base == 0), where
            if total:
                spans.append((base, total, d))
            written[base: base + total] = True
            o = 0
            for k, c in enumerate(cs):
                assert cont_info[b, d, k].tolist() == [o, len(c)], f"{where} contour {k}: cont_info {cont_info[b, d, k].tolist()}, expected {[o, len(c)]}"
                got = pts[b, base + o: base + o + len(c)].astype(np.int32)
                assert np.array_equal(got, c + [det.x0, det.y0]), f"{where} contour {k}: points differ"
                o += len(c)
            assert (cont_info[b, d, len(cs):] == INFO_CANARY).all(), f"{where}: cont_info written past contour {len(cs)}"
        assert n_full == full.get(b, 0), f"image {b}: {n_full} detections with status 4, the test arranged {full.get(b, 0)}"
        spans.sort()
        for (b0, t0, d0), (b1, _, d1) in zip(spans, spans[1:]):
            assert b0 + t0 <= b1, f"image {b}: the point blocks of detections {d0} and {d1} overlap"
        assert int(img_pts[b]) == sum(t for _, t, _ in spans), f"image {b}: image_points {int(img_pts[b])} != {sum(t for _, t, _ in spans)}"
        stray = np.flatnonzero((pts[b] != PTS_CANARY).any(axis=1) & ~written)
        assert stray.size == 0, f"image {b}: points written outside every traced block, first at {stray[:8].tolist()}"
    return seen
