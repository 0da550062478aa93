"""td_crown_zonal_dev (crownzonal.hip: a wave per crown, active-edge rows) against the exact oracle of zonal_cases.py on every
family, and against its host twin td_crown_zonal: status, count, minimum, maximum and position bit for bit; the same bits from a
raster that already lies on the device; nothing written outside the outputs; refusals leave them alone; n = 0 launches nothing.

Contract (zonal_cases.differing): selected values equal the oracle bit for bit (a NaN's payload aside); mean and variance lie within
one float32 ulp of the oracle's exact rational rounded once. The bound is derived, not tuned: any order of N float64 additions errs
by at most (N - 1) * 2^-53 * sum|v|; with N <= 2^15 pixels per crafted crown that is below 2^-38 * sum|v|. Every moment case has
values of one sign (sum|v| = |sum v|) and a spread of at least 2^-10 of the mean, so the kernel's float64 mean and variance — 64
lane sums joined by a butterfly — are within 2^-37 relatively of the exact ones, far under half a float32 ulp, and their float32
rounding is the once-rounded value or its neighbour. The constant case is exact (zonal_cases.moment_differs spells the steps out)."""
import ctypes as C

import numpy as np
import pytest
import torch

from treedetection_amd import _lib
from treedetection_amd import postprocessing as P
from treedetection_amd.cleaning import pack_rings

import zonal_cases as Z

pytestmark = pytest.mark.gpu

SENTINEL = -12345


def _dev(case, raster=None, kernel_only=False):
    """crown_zonal_stats on the GPU; ``kernel_only``: the kernel's own rows, the crowns over its capacity left at status 1."""
    raster = np.array(case.raster) if raster is None else raster
    if not kernel_only:
        return P.crown_zonal_stats(raster, case.transform, Z.launch_rings(case))
    st, out, pos, status = _direct(case)
    assert st == 0
    return out, pos[:, 0].copy(), pos[:, 1:].copy(), status


def _direct(case, pad=0, n=None, n_xy=None, rows=None, cols=None, null=None, misalign=False, start=None):
    """One td_crown_zonal_dev call, the three outputs views inside larger tensors of sentinels → (status code, out, pos, status) with
    the padding still on."""
    lib = _lib.load()
    xy, st_arr = pack_rings(Z.launch_rings(case))
    st_arr = st_arr if start is None else start
    k = st_arr.size - 1
    d_r = torch.from_numpy(np.array(case.raster)).cuda()
    d_xy = torch.from_numpy(np.concatenate([xy, np.zeros((1, 2))])).cuda()          # (one spare vertex: the misaligned view stays inside)
    d_st = torch.from_numpy(st_arr).cuda()
    d_o = torch.full((pad + 4 * k + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_p = torch.full((pad + 3 * k + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    d_s = torch.full((pad + k + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    ptr = {"raster": d_r.data_ptr(), "xy": d_xy.data_ptr() + (8 if misalign else 0), "start": d_st.data_ptr(), "out": d_o[pad:].data_ptr(),
           "pos": d_p[pad:].data_ptr(), "status": d_s[pad:].data_ptr()}
    if null:
        ptr[null] = None
    tr = (C.c_double * 6)(*case.transform)
    code = lib.td_crown_zonal_dev(ptr["raster"], case.raster.shape[0] if rows is None else rows, case.raster.shape[1] if cols is None else cols, tr,
                                  ptr["xy"], xy.shape[0] if n_xy is None else n_xy, ptr["start"], k if n is None else n, ptr["out"], ptr["pos"],
                                  ptr["status"], _lib.stream_ptr())
    torch.cuda.synchronize()
    out, pos, status = d_o.cpu().numpy(), d_p.cpu().numpy(), d_s.cpu().numpy()
    if pad == 0:
        return code, out.reshape(k, 4), pos.reshape(k, 3), status
    return code, out, pos, status


def _report(case, got, want):
    bad = np.flatnonzero(Z.differing(got, want))
    if not bad.size:
        return None
    k = int(bad[0])
    return (f"{case.name}: {bad.size} of {want.status.size} crowns differ, first crown {k}: got status {got[3][k]} count {got[1][k]} pos "
            f"{got[2][k].tolist()} stats {got[0][k].tolist()}, want status {want.status[k]} count {want.count[k]} pos {want.pos[k].tolist()} "
            f"stats {want.stats[k].tolist()}")


@pytest.mark.parametrize("family", list(Z.FAMILIES))
def test_kernel_equals_the_oracle_and_the_host_twin(family):
    report = []
    for i, case in enumerate(Z.cases(family)):
        want = Z.expected(family, i)
        got = _dev(case)
        host = P.crown_zonal_stats(np.array(case.raster), case.transform, Z.launch_rings(case), device=None)
        report.append(_report(case, got, want))
        stats, count, pos, status = got
        print(f"{family} {case.name}: {want.status.size} crowns, {int((status == 2).sum())} refused, counts {count[:12].tolist()}")
        # device and host twin: status, count, position, minimum and maximum bit for bit
        assert np.array_equal(status, host[3]) and np.array_equal(count, host[1]) and np.array_equal(pos, host[2])
        assert not (Z.selected_differs(stats[:, 0], host[0][:, 0]) | Z.selected_differs(stats[:, 1], host[0][:, 1])).any()
        # status 1 appears only where a ring is over the capacity, and only in the kernel's own rows: the wrapper has merged them
        kernel = _dev(case, kernel_only=True)
        over = np.array([r.shape[0] > Z.RING_CAP for r in Z.launch_rings(case)])
        assert np.array_equal(kernel[3] == 1, over) and (family == "capacity" or not over.any())
        assert np.isnan(kernel[0][over]).all() and (kernel[1][over] == -1).all() and (kernel[2][over] == -1).all()
        rest = ~over
        assert np.array_equal(Z._bits(kernel[0][rest]), Z._bits(stats[rest]))
        assert np.array_equal(kernel[1][rest], count[rest]) and np.array_equal(kernel[2][rest], pos[rest]) and np.array_equal(kernel[3][rest], status[rest])
        if "constant" in case.facts:                                  # known answer, exact: min = max = mean = the value, variance 0
            v = np.float32(case.facts["constant"])
            assert np.array_equal(Z._bits(stats), Z._bits(np.tile(np.array([v, v, v, 0.0], np.float32), (stats.shape[0], 1))))
        for group in case.facts.get("groups", []):                    # one ring, reversed / rotated / repeated: identical rows
            for j in group[1:]:
                assert np.array_equal(Z._bits(stats[group[0]]), Z._bits(stats[j])) and count[group[0]] == count[j] and (pos[group[0]] == pos[j]).all()
        if case.repeat is not None:                                   # a repeated ring gives the bits of its first copy, wherever the grid-stride loop takes it
            first = {}
            for k, j in enumerate(case.repeat):
                f = first.setdefault(int(j), k)
                assert np.array_equal(Z._bits(stats[f]), Z._bits(stats[k])) and count[f] == count[k] and (pos[f] == pos[k]).all()
    assert not any(report), "\n".join(r for r in report if r)


def test_a_raster_on_the_device_gives_the_same_bits():
    for family in ("clipping", "transforms"):
        for case in Z.cases(family):
            a, b = _dev(case), _dev(case, torch.from_numpy(np.array(case.raster)).cuda())
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b))
    with pytest.raises(ValueError, match="contiguous float32 CUDA tensor"):
        P.crown_zonal_stats(torch.zeros((4, 4), dtype=torch.float64, device="cuda"), Z.north_up(4), [Z.rect(0.2, 0.2, 3.8, 3.8)])


def test_nothing_is_written_outside_the_outputs():
    case = Z.cases("capacity")[0]
    want = Z.expected("capacity", 0)
    n, pad = len(case.rings), 64
    code, out, pos, status = _direct(case, pad=pad)
    assert code == 0
    for a, width in ((out, 4), (pos, 3), (status, 1)):
        assert (a[:pad] == SENTINEL).all() and (a[pad + width * n:] == SENTINEL).all() and a.size == 2 * pad + width * n
    st = status[pad:pad + n]
    assert st.tolist() == [1 if r.shape[0] > Z.RING_CAP else int(s) for r, s in zip(case.rings, want.status)]
    done = st == 0
    got = (out[pad:pad + 4 * n].reshape(n, 4)[done], pos[pad:pad + 3 * n].reshape(n, 3)[done, 0], pos[pad:pad + 3 * n].reshape(n, 3)[done, 1:], st[done])
    assert not Z.differing(got, Z.Expected(want.status[done], want.count[done], want.pos[done], want.stats[done])).any()


def test_starts_outside_xy_give_a_status_not_a_load():
    case = Z.cases("boundary")[0]
    m = [r.shape[0] for r in case.rings]
    good = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    _, out, pos, status = _direct(case)
    for start, refused in ((np.array([-1, *good[1:]], np.int64), 0), (np.array([*good[:-1], good[-1] + 1], np.int64), 3),
                           (np.array([good[0], good[2], good[1], *good[3:]], np.int64), 1), (np.array([-(2 ** 40), *good[1:]], np.int64), 0),
                           (np.array([*good[:-1], 2 ** 40], np.int64), 3)):
        code, o, p, s = _direct(case, start=start)
        assert code == 0 and s[refused] == 2 and np.isnan(o[refused]).all() and (p[refused] == -1).all()
        for k in range(len(m)):
            if k != refused and start[k] == good[k] and start[k + 1] == good[k + 1]:
                assert s[k] == 0 and np.array_equal(o[k], out[k]) and (p[k] == pos[k]).all()


def test_refusals_before_the_launch_leave_the_outputs_alone():
    case = Z.cases("boundary")[0]
    for kwargs in ({"null": "raster"}, {"null": "xy"}, {"null": "start"}, {"null": "out"}, {"null": "pos"}, {"null": "status"}, {"n": -1}, {"rows": 0},
                   {"cols": 0}, {"rows": -2}, {"n_xy": -1}, {"misalign": True}):
        code, out, pos, status = _direct(case, pad=8, **kwargs)
        assert code == _lib.ERR_INVALID and b"td_crown_zonal_dev" in _lib.load().td_last_error(), kwargs
        assert (out == SENTINEL).all() and (pos == SENTINEL).all() and (status == SENTINEL).all(), kwargs
    code, out, pos, status = _direct(case, pad=8, n=0)              # no crowns: fine, and nothing is launched or written
    assert code == 0 and (out == SENTINEL).all() and (pos == SENTINEL).all() and (status == SENTINEL).all()
    empty = P.crown_zonal_stats(np.array(case.raster), case.transform, [])
    assert [x.shape for x in empty] == [(0, 4), (0,), (0, 2), (0,)]
