"""td_crown_stats (crown.hip) against the brute-force oracle on the crafted rasters of crown_cases.py: values and positions as float32
bit patterns (NaN where the oracle has NaN), NDVI mean / variance within one float32 ulp of the oracle's float64 value rounded once;
the same bits from a raster that already lies on the device; nothing written outside ``out``; refusals leave ``out`` alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P

import crown_cases as CC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _selected_differs(got, want):
    """A max / min / position column: equal bits, or NaN on both sides (the payload is not part of the contract)."""
    return ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))


def _moment_differs(got, want):
    """mean / variance: within one float32 ulp of the expected value; NaN and inf by class and sign."""
    got64, want64 = got.astype(np.float64), want.astype(np.float64)
    finite = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(got) & (np.abs(got64 - want64) <= np.spacing(np.abs(want)).astype(np.float64))
    return ~np.where(finite, near, (np.isnan(want) & np.isnan(got)) | (np.isinf(want) & (got == want)))


def _differing_crowns(case, got, want):
    """→ bool [n]: crowns on which the kernel's row breaks the contract."""
    assert got.shape == want.shape and got.dtype == np.float32
    if case.mode == CC.HEIGHT:
        # the position always matches bits (the oracle's position is never NaN here)
        return _selected_differs(got[:, 0], want[:, 0]) | (_bits(got[:, 1:]) != _bits(want[:, 1:])).any(axis=1)
    bad = _selected_differs(got[:, 0], want[:, 0]) | _selected_differs(got[:, 1], want[:, 1])
    return bad | _moment_differs(got[:, 2], want[:, 2]) | _moment_differs(got[:, 3], want[:, 3])


def _run(case, raster=None):
    # (copies: the cases are read-only, and torch does not take read-only arrays quietly)
    return P.crown_stats(np.array(case.raster) if raster is None else raster, case.transform, case.bounds, np.array(case.circles), case.mode,
                         case.radius_scale)


@pytest.mark.parametrize("family,mode", CC.family_modes(), ids=lambda v: {0: "height", 1: "ndvi"}.get(v, v))
def test_crown_stats_equal_the_oracle(family, mode):
    report = []
    for i, case in enumerate(CC.cases(family)):
        if case.mode != mode:
            continue
        want = CC.expected(family, i)
        got = _run(case)
        bad = np.flatnonzero(_differing_crowns(case, got, want))
        print(f"{family} {case.name}: {bad.size} of {want.shape[0]} crowns differ")
        if bad.size:
            k = int(bad[0])
            report.append(f"{case.name}: {bad.size} of {want.shape[0]} crowns differ, first crown {k}: got {got[k].tolist()} want {want[k].tolist()}")
        if "constant" in case.facts:                         # known answer, exact: min = max = mean = the value, variance 0
            v = np.float32(case.facts["constant"])
            assert np.array_equal(_bits(got), _bits(np.tile(np.array([v, v, v, 0.0], np.float32), (got.shape[0], 1))))
        for group in case.facts.get("groups", []):           # duplicated circles: identical rows
            assert all(np.array_equal(_bits(got[group[0]]), _bits(got[j])) for j in group)
    assert not report, "\n".join(report)


@pytest.mark.parametrize("mode", [CC.HEIGHT, CC.NDVI], ids=["height", "ndvi"])
def test_a_raster_on_the_device_gives_the_same_bits(mode):
    for case in CC.cases("clipping"):
        if case.mode == mode:
            from_dev = _run(case, torch.from_numpy(np.array(case.raster)).cuda())
            assert np.array_equal(_bits(from_dev), _bits(_run(case)))


def _direct(case, out, n=None, window=None, mode=None):
    """One td_crown_stats call with ``out`` a float32 CUDA tensor VIEW (the kernel gets its data pointer) → status."""
    lib = _lib.load()
    rows, cols = case.raster.shape
    d_r = torch.from_numpy(np.array(case.raster)).cuda()
    d_c = torch.from_numpy(np.array(case.circles)).cuda()
    r_lo, c_lo, r_hi, c_hi = P._window(case.transform, rows, cols, case.bounds)
    win = (C.c_int32 * 4)(*(window or (r_lo, c_lo, min(r_hi, rows - 1), min(c_hi, cols - 1))))
    tr = (C.c_double * 6)(*case.transform)
    st = lib.td_crown_stats(d_r.data_ptr(), rows, cols, tr, win, d_c.data_ptr(), case.circles.shape[0] if n is None else n,
                            case.mode if mode is None else mode, case.radius_scale, out.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("mode", [CC.HEIGHT, CC.NDVI], ids=["height", "ndvi"])
def test_nothing_is_written_outside_out(mode):
    """``out`` sits inside a larger tensor of sentinels, n * 3 (n * 4) floats wide: the sentinels on both sides stay intact."""
    i, case = next((i, c) for i, c in enumerate(CC.cases("clipping")) if c.mode == mode)
    n, width, pad = case.circles.shape[0], 4 if mode else 3, 64
    big = torch.full((pad + n * width + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    assert _direct(case, big[pad:pad + n * width]) == 0
    host = big.cpu().numpy()
    assert (host[:pad] == SENTINEL).all() and (host[pad + n * width:] == SENTINEL).all()
    assert not _differing_crowns(case, host[pad:pad + n * width].reshape(n, width), CC.expected("clipping", i)).any()


def test_refusals_leave_out_untouched():
    case = next(c for c in CC.cases("clipping") if c.mode == CC.NDVI)
    rows, cols = case.raster.shape
    n = case.circles.shape[0]
    out = torch.full((n * 4,), SENTINEL, dtype=torch.float32, device="cuda")
    for kwargs in ({"window": (0, 0, rows, cols - 1)}, {"window": (0, 0, rows - 1, cols)}, {"window": (-1, 0, rows - 1, cols - 1)},
                   {"window": (0, -1, rows - 1, cols - 1)}, {"mode": 2}, {"mode": -1}):
        assert _direct(case, out, **kwargs) < 0, kwargs
        assert (out.cpu().numpy() == SENTINEL).all(), kwargs
    assert _direct(case, out, n=0) == 0                      # no crowns: fine, and nothing to write
    assert (out.cpu().numpy() == SENTINEL).all()
