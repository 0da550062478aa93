"""Shared inputs of the crown-label tests (test_label_cases.py, test_crown_labels_gpu.py, test_postprocessing_labels_gpu.py): what a
label raster must hold, built from the exact oracle of zonal_cases.py alone. Not a test.

NO EXPECTATION COMES FROM THE CODE UNDER TEST. For the families of zonal_cases.FAMILIES the pixels of every ring are
``zonal_cases.inside(family, i)`` — exact rational membership on the float64 centres —; for the overlap cases below they are
``zonal_cases.pixels_inside`` on the same centres. The raster is those sets composited in numpy by the rule of include/treedet.h:
``labels = max(labels before, value)`` over the pixels of every ring that is drawn, an UNSIGNED maximum. Refused rings (status 2)
draw nothing; for a kernel-only run (``kernel_only``) the rings over zonal_cases.RING_CAP draw nothing either and have status 1.

``label_cases()`` → every case: each case of each zonal family with seeded uint32 values, then the overlap cases the families lack
(rasters at most 140 x 140):
  crossing        two crossing rings, the higher value listed first, and listed last
  equal           equal values on crossing rings
  zero_between    a value of 0 on a ring between two others
  sign_bit        0x7FFFFFFF, 0x80000000 and 0xFFFFFFFF on overlapping rings, in three orders (a signed maximum gets these wrong)
  many_waves      one ring repeated more than IN_FLIGHT times with distinct values: waves of different workgroups and loop turns meet
                  on the same pixels
  prefilled       labels that hold values already: inside a ring some larger and some smaller than the ring's, a pattern outside
"""
import functools
from typing import Any, List, NamedTuple, Optional, Tuple

import numpy as np

import zonal_cases as Z


class LabelCase(NamedTuple):
    name: str
    shape: Tuple[int, int]
    transform: Tuple[float, ...]
    rings: Tuple[np.ndarray, ...]         # what the launch sees (repeats expanded), float64 [m, 2], open
    values: np.ndarray                    # uint32 [n]
    pixels: Any                           # per ring of the launch the (row, col) pairs inside, from the oracle
    before: Optional[np.ndarray]          # uint32 [rows, cols] the labels hold before the call, or None: zeros


def values_for(n, seed):
    """n seeded uint32 values over the whole range, none 0; every eighth equal to its predecessor, so that equal values meet."""
    v = np.random.default_rng(seed).integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v[8::8] = v[7:-1:8][:v[8::8].size]
    return Z._frozen(v)


def _overlap(name, rows, cols, rings, values, repeat=None, before=None):
    t = Z.north_up(rows)
    X, Y = Z.centres(t, rows, cols)
    rings = [Z._frozen(np.asarray(r, dtype=np.float64).reshape(-1, 2)) for r in rings]
    pix = [Z.pixels_inside(r, X, Y) for r in rings]
    if repeat is not None:
        rings, pix = [rings[j] for j in repeat], [pix[j] for j in repeat]
    values = Z._frozen(np.asarray(values, dtype=np.uint32))
    assert rows <= 140 and cols <= 140 and values.shape == (len(rings),)
    return LabelCase(name, (rows, cols), t, tuple(rings), values, pix, None if before is None else Z._frozen(before))


def _overlap_cases() -> List[LabelCase]:
    a, b = Z.rect(2.2, 8.3, 27.8, 15.7), Z.rect(11.3, 1.2, 18.6, 28.9)                 # a cross: 7 x 7 shared centres
    tri = [(3.3, 3.1), (28.4, 9.9), (6.2, 27.7)]
    out = [_overlap("crossing_high_first", 30, 30, [a, b], [9, 4]), _overlap("crossing_high_last", 30, 30, [a, b], [4, 9]),
           _overlap("equal", 30, 30, [a, b, tri], [7, 7, 7]), _overlap("zero_between", 30, 30, [a, tri, b], [5, 0, 3]),
           _overlap("zero_alone", 30, 30, [tri], [0])]
    big = (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
    for k, order in enumerate(((0, 1, 2), (2, 1, 0), (1, 2, 0))):
        out.append(_overlap(f"sign_bit_{k}", 30, 30, [a, b, tri], [big[j] for j in order]))
    # one ring, more copies than a launch holds in flight, distinct values in a seeded order; a second ring crosses it
    n = Z.IN_FLIGHT + 301
    vals = np.random.default_rng(31).permutation(n).astype(np.uint32) + 1
    star = Z.star(np.random.default_rng(32), 20.0, 20.0, 6.0, 17.0, 23)
    out.append(_overlap("many_waves", 40, 40, [star, Z.rect(1.2, 17.3, 38.8, 22.6)], np.concatenate([vals, [n // 2]]),
                        repeat=np.concatenate([np.zeros(n, np.int64), [1]])))
    # labels that hold values already
    rows = cols = 36
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    before = (1000 + 37 * rr + cc).astype(np.uint32)                                   # a pattern, every pixel its own value
    before[(rr + cc) % 3 == 0] = 0xF0000000 + 5                                        # larger than any value drawn
    before[(rr + cc) % 3 == 1] = 2                                                     # smaller
    out.append(_overlap("prefilled", rows, cols, [Z.rect(4.2, 5.3, 30.8, 19.7), Z.rect(12.3, 9.2, 24.6, 33.9), tri], [5000, 0x90000000, 3],
                        before=before))
    return out


@functools.lru_cache(maxsize=None)
def label_cases() -> Tuple[LabelCase, ...]:
    out = []
    for fi, family in enumerate(Z.FAMILIES):
        for i, case in enumerate(Z.cases(family)):
            rings = Z.launch_rings(case)
            out.append(LabelCase(f"{family}/{case.name}", case.raster.shape, case.transform, tuple(rings), values_for(len(rings), 100 * fi + i),
                                 Z.inside(family, i), None))
    return tuple(out + _overlap_cases())


def before(case: LabelCase) -> np.ndarray:
    """A fresh copy of what the labels hold before the call."""
    return np.zeros(case.shape, np.uint32) if case.before is None else np.array(case.before)


def composite(shape, pixels, values, drawn, start=None, rule=np.maximum) -> np.ndarray:
    """The rule, in numpy: ``rule`` (the unsigned maximum) of the labels so far and ``values[k]`` over ``pixels[k]`` for every k in
    ``drawn``."""
    out = np.zeros(shape, np.uint32) if start is None else np.array(start, dtype=np.uint32)
    for k in drawn:
        if pixels[k]:
            rr, cc = np.array(pixels[k]).T
            out[rr, cc] = rule(out[rr, cc], np.uint32(values[k]))
    return out


def expected(case: LabelCase, kernel_only=False):
    """→ (labels uint32 [rows, cols], status int32 [n]) the call must leave."""
    status = np.array([2 if Z.refused(r) else (1 if kernel_only and r.shape[0] > Z.RING_CAP else 0) for r in case.rings], np.int32)
    return composite(case.shape, case.pixels, case.values, np.flatnonzero(status == 0), before(case)), status


def report(case: LabelCase, got, want) -> Optional[str]:
    """None when labels and status equal the expectation, pixel for pixel; else what differs first."""
    (labels, status), (w_labels, w_status) = got, want
    assert labels.dtype == np.uint32 and labels.shape == w_labels.shape and status.shape == w_status.shape, (case.name, labels.dtype, labels.shape)
    msg = []
    bad = np.argwhere(labels != w_labels)
    if bad.size:
        r, c = bad[0]
        msg.append(f"{bad.shape[0]} of {labels.size} pixels differ, first ({r}, {c}): got {labels[r, c]:#x}, want {w_labels[r, c]:#x}")
    sbad = np.flatnonzero(status != w_status)
    if sbad.size:
        msg.append(f"{sbad.size} statuses differ, first ring {sbad[0]}: got {status[sbad[0]]}, want {w_status[sbad[0]]}")
    return f"{case.name}: " + "; ".join(msg) if msg else None


def expected_from_layer(shape, transform, rings, scores) -> np.ndarray:
    """The label raster of a processed layer, from its rings (closed, as read back) and scores: label k + 1 on the pixels the oracle
    puts inside ring k; where crowns overlap, the higher score wins and among equal scores the lower index — a sort written out."""
    X, Y = Z.centres(transform, *shape)
    order = sorted(range(len(rings)), key=lambda k: (scores[k], -k))                   # worst first: later ones paint over
    out = np.zeros(shape, np.uint32)
    for k in order:
        ring = np.asarray(rings[k], dtype=np.float64)
        ring = ring[:-1] if (ring[0] == ring[-1]).all() else ring
        for r, c in Z.pixels_inside(ring, X, Y):
            out[r, c] = k + 1
    return out
