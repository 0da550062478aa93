"""td_crown_labels_dev (crownzonal.hip: the zonal walk, drawing with one atomic maximum per pixel) against the expectation of
label_cases.py — the exact oracle's pixel sets composited by the unsigned maximum in numpy — on every family of
zonal_cases.FAMILIES and every overlap case, pixel for pixel and status for status; against its host twin on random overlapping
stars; the merged host fallback for rings over the kernel's capacity; nothing written outside the outputs; refusals leave them
alone; n = 0 launches nothing; ``out=`` on the device is used where it lies."""
import ctypes as C

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P
from treedetection_amd.cleaning import pack_rings

import label_cases as L
import zonal_cases as Z

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 64


def _direct(case, pad=0, n=None, n_xy=None, rows=None, cols=None, null=None, misalign=False, start=None, transform=None):
    """One td_crown_labels_dev call over ``before(case)``, labels and status views inside larger tensors of sentinels →
    (status code, labels, status), flat with the padding still on when ``pad`` > 0."""
    lib = _lib.load()
    xy, st_arr = pack_rings(list(case.rings))
    st_arr = st_arr if start is None else start
    k = st_arr.size - 1
    R, Cc = case.shape
    d_xy = torch.from_numpy(np.concatenate([xy, np.zeros((1, 2))])).cuda()          # (one spare vertex: the misaligned view stays inside)
    d_st = torch.from_numpy(st_arr).cuda()
    d_v = torch.from_numpy(np.concatenate([case.values, [0]]).astype(np.uint32).view(np.int32)).cuda()
    d_l = torch.full((pad + R * Cc + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    d_l[pad:pad + R * Cc] = torch.from_numpy(L.before(case).view(np.int32).reshape(-1)).cuda()
    d_s = torch.full((pad + k + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    ptr = {"xy": d_xy.data_ptr() + (8 if misalign else 0), "start": d_st.data_ptr(), "value": d_v.data_ptr(), "labels": d_l[pad:].data_ptr(),
           "status": d_s[pad:].data_ptr(), "transform": (C.c_double * 6)(*(case.transform if transform is None else transform))}
    if null:
        ptr[null] = None
    code = lib.td_crown_labels_dev(R if rows is None else rows, Cc if cols is None else cols, ptr["transform"], ptr["xy"],
                                   xy.shape[0] if n_xy is None else n_xy, ptr["start"], ptr["value"], k if n is None else n, ptr["labels"], ptr["status"],
                                   _lib.stream_ptr())
    torch.cuda.synchronize()
    labels, status = d_l.cpu().numpy().view(np.uint32), d_s.cpu().numpy()
    if pad == 0:
        return code, labels.reshape(R, Cc), status
    return code, labels, status


def _of_family(family):
    return [c for c in L.label_cases() if c.name.startswith(family + "/")]


@pytest.mark.parametrize("family", list(Z.FAMILIES) + ["overlap"])
def test_kernel_equals_the_expected_raster(family):
    cases = [c for c in L.label_cases() if "/" not in c.name] if family == "overlap" else _of_family(family)
    assert cases
    reports = []
    for case in cases:
        want = L.expected(case, kernel_only=True)
        code, labels, status = _direct(case)
        assert code == 0
        print(f"{case.name}: {len(case.rings)} rings on {case.shape}, {int((want[0] != L.before(case)).sum())} pixels change, statuses "
              f"{np.bincount(want[1], minlength=3).tolist()}")
        reports.append(L.report(case, (labels, status), want))
    assert not any(reports), "\n".join(r for r in reports if r)


def test_what_the_families_must_include_is_there():
    names = [c.name for c in L.label_cases()]
    assert "transforms/rotated" in names and "lanes/widths" in names and "capacity/at_and_over" in names and "lanes/grid_stride" in names
    cap = next(c for c in L.label_cases() if c.name == "capacity/at_and_over")
    sizes = [r.shape[0] for r in cap.rings]
    assert Z.RING_CAP in sizes and Z.RING_CAP + 1 in sizes and _lib.ZONAL_RING_CAP == Z.RING_CAP
    want = L.expected(cap, kernel_only=True)[1]
    assert want[sizes.index(Z.RING_CAP)] == 0 and want[sizes.index(Z.RING_CAP + 1)] == 1 and (want == 2).sum() == 5
    widths = next(c for c in L.label_cases() if c.name == "lanes/widths")
    assert [len(p) // 3 for p in widths.pixels[:5]] == [1, 63, 64, 65, 129]
    many = next(c for c in L.label_cases() if c.name == "many_waves")
    assert len(many.rings) > Z.IN_FLIGHT


def test_rings_over_the_capacity_are_drawn_by_the_merged_host_fallback():
    cap = next(c for c in L.label_cases() if c.name == "capacity/at_and_over")
    over = [k for k, r in enumerate(cap.rings) if r.shape[0] > Z.RING_CAP]
    assert over
    kernel, whole = L.expected(cap, kernel_only=True), L.expected(cap)
    assert (kernel[0] != whole[0]).any()                      # the over-cap rings own pixels of their own
    labels, status = P.crown_label_raster(list(cap.rings), cap.values, cap.transform, cap.shape)
    assert L.report(cap, (labels, status), whole) is None
    # and into a tensor that lies on the device already, over what it holds
    pre = next(c for c in L.label_cases() if c.name == "prefilled")
    rings = list(pre.rings) + [cap.rings[over[0]] + 9.0]
    values = np.concatenate([pre.values, [0xA0000000]]).astype(np.uint32)
    X, Y = Z.centres(pre.transform, *pre.shape)
    extra = L.LabelCase("prefilled+over", pre.shape, pre.transform, tuple(rings), values, list(pre.pixels) + [Z.pixels_inside(rings[-1], X, Y)],
                                pre.before)
    assert len(extra.pixels[-1]) > 20
    d_out = torch.from_numpy(L.before(extra).view(np.int32)).cuda()
    got, status = P.crown_label_raster(rings, values, pre.transform, pre.shape, out=d_out)
    assert got is d_out and status.tolist() == [0, 0, 0, 0]
    assert L.report(extra, (d_out.cpu().numpy().view(np.uint32), status), L.expected(extra)) is None


def test_device_equals_the_host_twin_on_random_overlapping_stars():
    rng = np.random.default_rng(77)
    rows = cols = 200
    for t in ((0.2, 0.0, Z.UTM_X, 0.0, -0.2, Z.UTM_Y), (0.2 * np.cos(0.07), 0.2 * np.sin(0.07), Z.UTM_X, 0.2 * np.sin(0.07), -0.2 * np.cos(0.07), Z.UTM_Y)):
        X, Y = Z.centres(t, rows, cols)
        rings = []
        for _ in range(300):
            r, c = rng.integers(-5, rows + 5), rng.integers(-5, cols + 5)
            cx, cy = t[0] * (c + 0.5) + t[1] * (r + 0.5) + t[2], t[3] * (c + 0.5) + t[4] * (r + 0.5) + t[5]
            rings.append(Z.star(rng, cx, cy, 0.4, 6.0, int(rng.integers(3, 60))))
        values = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
        values[::7] = values[3]                                # equal values meet
        values[5::40] = 0
        before = rng.integers(0, 1 << 30, (rows, cols), dtype=np.uint64).astype(np.uint32) * (rng.random((rows, cols)) < 0.3)
        host, h_status = P.crown_label_raster(rings, values, t, (rows, cols), device=None, out=before.copy())
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        dev, d_status = P.crown_label_raster(rings, values, t, (rows, cols), out=d_out)
        got = dev.cpu().numpy().view(np.uint32)
        changed = int((host != before).sum())
        print(f"b = {t[1]:.3f}: {changed} of {rows * cols} pixels change, {np.unique(host).size} distinct labels")
        assert changed > 10000 and np.array_equal(h_status, d_status) and (h_status == 0).all()
        assert np.array_equal(got, host), f"{int((got != host).sum())} pixels differ between device and host"
        # a fresh raster through the wrapper's own allocation: zeros underneath
        fresh, _ = P.crown_label_raster(rings, values, t, (rows, cols))
        zero_host, _ = P.crown_label_raster(rings, values, t, (rows, cols), device=None)
        assert fresh.dtype == np.uint32 and np.array_equal(fresh, zero_host)


def test_nothing_is_written_outside_the_outputs():
    for name in ("capacity/at_and_over", "clipping/9x11", "prefilled", "transforms/rotated"):
        case = next(c for c in L.label_cases() if c.name == name)
        n, px = len(case.rings), case.shape[0] * case.shape[1]
        code, labels, status = _direct(case, pad=PAD)
        assert code == 0 and labels.size == 2 * PAD + px and status.size == 2 * PAD + n
        assert (labels[:PAD] == SENTINEL).all() and (labels[PAD + px:] == SENTINEL).all()
        assert (status[:PAD] == SENTINEL).all() and (status[PAD + n:] == SENTINEL).all()
        got = (labels[PAD:PAD + px].reshape(case.shape), status[PAD:PAD + n])
        assert L.report(case, got, L.expected(case, kernel_only=True)) is None


def test_prefilled_labels_are_composited_over():
    case = next(c for c in L.label_cases() if c.name == "prefilled")
    code, labels, status = _direct(case)
    want, _ = L.expected(case)
    assert code == 0 and np.array_equal(labels, want)
    outside = L.composite(case.shape, case.pixels, np.ones(3, np.uint32), [0, 1, 2]) == 0
    assert outside.any() and np.array_equal(labels[outside], case.before[outside])
    assert (labels >= case.before).all() and (labels > case.before).any() and (labels[~outside] == case.before[~outside]).any()


def test_starts_outside_xy_give_a_status_not_a_load():
    case = next(c for c in L.label_cases() if c.name == "boundary/on_centres")
    m = [r.shape[0] for r in case.rings]
    good = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    for start, refused in ((np.array([-1, *good[1:]], np.int64), 0), (np.array([*good[:-1], good[-1] + 1], np.int64), 3),
                           (np.array([good[0], good[2], good[1], *good[3:]], np.int64), 1), (np.array([-(2 ** 40), *good[1:]], np.int64), 0),
                           (np.array([*good[:-1], 2 ** 40], np.int64), 3)):
        code, labels, status = _direct(case, start=start)
        intact = [k for k in range(len(m)) if start[k] == good[k] and start[k + 1] == good[k + 1]]
        assert code == 0 and status[refused] == 2 and all(status[k] == 0 for k in intact)
        assert refused not in intact
        drawn = [k for k in range(len(m)) if status[k] == 0]
        assert set(intact) <= set(drawn)
        if set(drawn) == set(intact):
            assert np.array_equal(labels, L.composite(case.shape, case.pixels, case.values, intact))


def test_refusals_before_the_launch_leave_the_outputs_alone():
    case = next(c for c in L.label_cases() if c.name == "prefilled")
    px = case.shape[0] * case.shape[1]
    nan_t = [list(case.transform) for _ in range(3)]
    nan_t[0][0], nan_t[1][5], nan_t[2][1] = float("nan"), float("inf"), float("-inf")
    for kwargs in ({"null": "transform"}, {"null": "xy"}, {"null": "start"}, {"null": "value"}, {"null": "labels"}, {"null": "status"}, {"n": -1},
                   {"rows": 0}, {"cols": 0}, {"rows": -2}, {"n_xy": -1}, {"misalign": True}, {"rows": 1 << 16, "cols": 1 << 15},
                   {"transform": nan_t[0]}, {"transform": nan_t[1]}, {"transform": nan_t[2]}):
        code, labels, status = _direct(case, pad=8, **kwargs)
        assert code == _lib.ERR_INVALID and b"td_crown_labels_dev" in _lib.load().td_last_error(), kwargs
        assert (labels[:8] == SENTINEL).all() and (labels[8 + px:] == SENTINEL).all() and (status == SENTINEL).all(), kwargs
        assert np.array_equal(labels[8:8 + px].reshape(case.shape), case.before), kwargs
    code, labels, status = _direct(case, pad=8, n=0)              # no crowns: fine, and nothing is launched or written
    assert code == 0 and np.array_equal(labels[8:8 + px].reshape(case.shape), case.before) and (status == SENTINEL).all()
    empty, st = P.crown_label_raster([], [], case.transform, (5, 7))
    assert empty.shape == (5, 7) and empty.dtype == np.uint32 and not empty.any() and st.shape == (0,)


def test_out_on_the_device_is_used_where_it_lies():
    case = next(c for c in L.label_cases() if c.name == "sign_bit_0")
    big = torch.full((case.shape[0] + 2, case.shape[1]), 77, dtype=torch.int32, device="cuda")
    view = big[1:-1]                                            # contiguous rows inside a larger tensor
    view.zero_()
    ptr = view.data_ptr()
    got, status = P.crown_label_raster(list(case.rings), case.values, case.transform, case.shape, out=view)
    assert got is view and got.data_ptr() == ptr and got.is_cuda and status.tolist() == [0, 0, 0]
    assert np.array_equal(view.cpu().numpy().view(np.uint32), L.expected(case)[0])
    assert (big[0] == 77).all() and (big[-1] == 77).all()
    # a second call composites over the first
    other = next(c for c in L.label_cases() if c.name == "crossing_high_first")
    P.crown_label_raster(list(other.rings), other.values, other.transform, other.shape, out=view)
    both = L.composite(case.shape, other.pixels, other.values, [0, 1], L.expected(case)[0])
    assert np.array_equal(view.cpu().numpy().view(np.uint32), both)
    # the priorities of a layer go back to labels on the device, in place of nothing larger than the raster
    priority, table = P.crown_priorities([0.5, 0.9, 0.9])
    d_p = torch.zeros(case.shape, dtype=torch.int32, device="cuda")
    P.crown_label_raster(list(case.rings), priority, case.transform, case.shape, out=d_p)
    lab = P.labels_from_priorities(d_p, table)
    assert lab.is_cuda and lab.dtype == torch.int32 and lab.shape == d_p.shape
    want = L.expected_from_layer(case.shape, case.transform, list(case.rings), [0.5, 0.9, 0.9])
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), want)
    for bad in (torch.zeros(case.shape, dtype=torch.int64, device="cuda"), torch.zeros((3, 3), dtype=torch.int32, device="cuda"),
                torch.zeros(case.shape, dtype=torch.int32), np.zeros(case.shape, np.uint32)):
        with pytest.raises(ValueError, match="contiguous int32 / uint32 CUDA tensor"):
            P.crown_label_raster(list(case.rings), case.values, case.transform, case.shape, out=bad)
