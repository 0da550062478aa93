"""td_treetops_dev (treetops.hip: both smoothing passes, the window maximum and the comparison of a tile in LDS) against its host
twin td_treetops bit for bit — marks, smoothed raster, counts = the marks' row sums — on every case of tests/treetop_cases.py within
the kernel's caps (both tile sizes, rasters smaller than the halo, tile edges, plateaus, NaN and infinite pixels), against the
recorded scipy results, with nothing written outside the outputs; a tensor raster is read in place; parameters over a cap go to
the host twin and agree; malformed calls are refused before anything is written."""
import numpy as np
import pytest
import torch

import treetop_cases as tc
from treedetection_amd import _lib, treetops as tt

pytestmark = pytest.mark.gpu

PAD = 256


def device_direct(raster, w, k, floor, smoothed=True, counts=True):
    """One td_treetops_dev call with every output inside a larger tensor of sentinels → (marks, smoothed, counts) on the host."""
    rows, cols = raster.shape
    w = np.ascontiguousarray(w, np.float64)
    d_r = torch.from_numpy(np.ascontiguousarray(raster, np.float32)).cuda()
    d_m = torch.full((PAD + rows * cols + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    d_s = torch.full((PAD + rows * cols + PAD,), -12345.0, dtype=torch.float32, device="cuda")
    d_c = torch.full((PAD + rows + PAD,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().td_treetops_dev(d_r.data_ptr(), rows, cols, w.ctypes.data, (w.size - 1) // 2, k, float(floor), d_m[PAD:].data_ptr(),
                                           d_s[PAD:].data_ptr() if smoothed else None, d_c[PAD:].data_ptr() if counts else None,
                                           _lib.stream_ptr()), "td_treetops_dev")
    m, s, c = d_m.cpu().numpy(), d_s.cpu().numpy(), d_c.cpu().numpy()
    assert (m[:PAD] == 0x5A).all() and (m[-PAD:] == 0x5A).all() and (s[:PAD] == -12345.0).all() and (s[-PAD:] == -12345.0).all()
    assert (c[:PAD] == -7).all() and (c[-PAD:] == -7).all()
    if not smoothed:
        assert (s == -12345.0).all()
    if not counts:
        assert (c == -7).all()
    return m[PAD:-PAD].reshape(rows, cols), s[PAD:-PAD].reshape(rows, cols), c[PAD:-PAD]


def check_against_host(name, raster, w, k, floor):
    marks, smoothed, counts = device_direct(raster, w, k, floor)
    want_marks, want_smoothed, want_counts = tt._run(np.ascontiguousarray(raster, np.float32), w, k, floor, None, True, True, "test")
    assert tc.same_floats(smoothed, want_smoothed), name
    assert (marks == want_marks).all(), (name, np.argwhere(marks != want_marks)[:5])
    assert (counts == want_counts).all() and (counts == want_marks.sum(axis=1)).all(), name
    return marks


@pytest.mark.parametrize("shape", tc.SHAPES, ids=[f"{r}x{c}" for r, c in tc.SHAPES])
def test_device_equals_the_host_twin_on_random_and_plateau_rasters(shape):
    for name, raster, w, k, floor in tc.random_cases(shape):
        check_against_host(name, raster, w, k, floor)


def test_device_equals_the_host_twin_on_crafted_rasters():
    for name, raster, w, k, floor, expected in tc.crafted_cases():
        marks = check_against_host(name, raster, w, k, floor)
        if expected is not None:
            assert sorted(map(tuple, np.argwhere(marks))) == sorted(expected), name


def test_optional_outputs_are_optional():
    name, raster, w, k, floor = tc.random_cases((65, 129))[13]
    full = device_direct(raster, w, k, floor)
    assert (device_direct(raster, w, k, floor, smoothed=False, counts=False)[0] == full[0]).all()
    assert (device_direct(raster, w, k, floor, smoothed=False)[2] == full[2]).all()


def test_device_equals_the_recorded_scipy_results():
    for name, raster, sigma, k, floor, smoothed, tops in tc.golden_cases():
        assert tc.same_floats(tt.smooth_height(raster, sigma, device=0).cpu().numpy(), smoothed), name
        rows, cols, height, _ = tt.find_treetops(raster, None, sigma, k, floor, device=0)
        assert (np.stack([rows, cols], axis=1).reshape(-1, 2) == tops.reshape(-1, 2)).all(), name
        assert tc.same_floats(height, smoothed[tops[:, 0], tops[:, 1]]), name


def test_a_tensor_raster_is_read_in_place():
    raster = tc.canopy((70, 131), 5, plateaus=True)
    d_r = torch.from_numpy(raster).cuda()
    before = d_r.clone()
    marks, smoothed, counts = tt.treetop_marks(d_r, smoothed=True, counts=True)
    assert marks.is_cuda and marks.dtype == torch.uint8 and smoothed.is_cuda and counts.dtype == torch.int32 and torch.equal(d_r, before)
    want = tt.treetop_marks(raster, device=None, smoothed=True, counts=True)
    assert (marks.cpu().numpy() == want[0]).all() and tc.same_floats(smoothed.cpu().numpy(), want[1]) and (counts.cpu().numpy() == want[2]).all()
    t = (0.5, 0.0, 100.0, 0.0, -0.5, 200.0)
    got, ref = tt.find_treetops(d_r, t), tt.find_treetops(raster, t, device=None)
    assert len(ref[0]) > 50 and all((a == b).all() for a, b in zip(got, ref))
    for bad in (d_r.double(), d_r[:, ::2], d_r.cpu()[None]):
        with pytest.raises(ValueError):
            tt.treetop_marks(bad)


def test_parameters_over_a_cap_go_to_the_host_twin(capsys):
    raster = tc.canopy((40, 50), 6, plateaus=False)
    d_r = torch.from_numpy(raster).cuda()
    for sigma, k in ((2.5, 7), (0.5, 17)):                  # radius 10 > 8; window 17 > 15
        marks = tt.treetop_marks(d_r, sigma=sigma, window=k)
        assert "using the host function" in capsys.readouterr().out
        assert marks.is_cuda and (marks.cpu().numpy() == tt.treetop_marks(raster, sigma=sigma, window=k, device=None)).all()
        assert (marks.cpu().numpy() == tc.oracle(raster, tc.weights(sigma), k, 3.0)[0]).all()
    w = tc.weights(2.5)
    marks = torch.zeros((40, 50), dtype=torch.uint8, device="cuda")
    assert _lib.load().td_treetops_dev(d_r.data_ptr(), 40, 50, w.ctypes.data, 10, 7, 3.0, marks.data_ptr(), None, None, _lib.stream_ptr()) == _lib.ERR_INVALID
    assert b"radius 10" in _lib.load().td_last_error()


def test_malformed_device_calls_are_refused_before_anything_runs():
    lib = _lib.load()
    d_r = torch.ones((4, 5), dtype=torch.float32, device="cuda")
    marks = torch.full((4, 5), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    good = np.ascontiguousarray(tc.weights(0.5))

    def call(r=d_r.data_ptr(), rows=4, cols=5, wt=good, radius=2, window=7, floor=3.0, m=marks.data_ptr()):
        wt = None if wt is None else np.ascontiguousarray(wt, np.float64)
        return lib.td_treetops_dev(r, rows, cols, None if wt is None else wt.ctypes.data, radius, window, floor, m, None, counts.data_ptr(),
                                   _lib.stream_ptr())

    bad = dict(r=dict(r=None), w=dict(wt=None), m=dict(m=None), rows=dict(rows=0), cols=dict(cols=-1), pixels=dict(rows=1 << 16, cols=1 << 15),
               even=dict(window=6), zero=dict(window=0), radius=dict(radius=-1), floor=dict(floor=float("nan")), over_window=dict(window=17),
               over_radius=dict(radius=9, wt=np.ones(19) / 19), nan_weight=dict(wt=[0.1, np.nan, 0.8, np.nan, 0.1]),
               asymmetric=dict(wt=[0.1, 0.2, 0.4, 0.2, 0.15]))
    for name, kw in bad.items():
        assert call(**kw) == _lib.ERR_INVALID, name
        assert lib.td_last_error().startswith(b"td_treetops_dev:"), name
    torch.cuda.synchronize()
    assert (marks == 7).all() and (counts == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (marks == 0).all() and (counts == 0).all()       # a flat raster of 1 m: below the floor
