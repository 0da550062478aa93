"""The case families of crown_cases.py do what their names say — shown with oracle.postprocess_ref alone, no kernel and no GPU."""
import numpy as np
import pytest

from oracle import postprocess_ref as O

import crown_cases as CC

ALL = [(fam, i) for fam in CC.FAMILIES for i in range(len(CC.cases(fam)))]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("family", list(CC.FAMILIES))
def test_vertex_helper_reproduces_every_circle_bit_for_bit(family):
    for case in CC.cases(family):
        assert case.raster.dtype == np.float32 and case.circles.dtype == np.float32 and case.raster.shape[0] <= 400 and case.raster.shape[1] <= 400
        for k, (px, py) in enumerate(zip(*CC.vertices(case.circles))):
            assert px.dtype == np.float32 and py.dtype == np.float32
            got = np.array(O._circle(px, py), dtype=np.float32)
            assert np.array_equal(_bits(got), _bits(case.circles[k])), (case.name, k, got, case.circles[k])


@pytest.mark.parametrize("family,i", ALL)
def test_inside_masks_reproduce_the_oracle_results(family, i):
    """crown_cases.inside_masks restates the oracle's membership test; the values it selects are the oracle's results."""
    case, want = CC.cases(family)[i], CC.expected(family, i)
    masks, xs, ys, flat = CC.inside_masks(case)
    assert want.shape == (case.circles.shape[0], 4 if case.mode else 3)
    with np.errstate(all="ignore"):
        for k in range(case.circles.shape[0]):
            v = flat[masks[k]]
            if v.size == 0:
                assert (want[k] == -1).all()
            elif case.mode == CC.HEIGHT:
                j = int(np.argmax(v))
                assert np.array_equal(_bits([v[j], xs[masks[k]][j], ys[masks[k]][j]]), _bits(want[k]))
            else:
                assert np.array_equal(_bits([v.min(), v.max()]), _bits(want[k, :2]))


@pytest.mark.parametrize("family,i", ALL)
def test_the_modelled_kernel_box_holds_every_oracle_inside_pixel(family, i):
    """crown_cases.kernel_box restates the box arithmetic of crown.hip, NDVI mode's float32 rounding margin included: on every case no
    pixel the oracle counts lies outside it, and on an axis-aligned raster the box stays of the circle's size, not the subset's."""
    case = CC.cases(family)[i]
    masks = CC.inside_masks(case)[0]
    sub_rows, sub_cols = CC.window(case)[2:]
    a, b, _, d, e, _ = case.transform
    for k in range(case.circles.shape[0]):
        r0, c0, bh, bw = CC.kernel_box(case, k)
        lin = np.flatnonzero(masks[k])
        rs, cs = lin // sub_cols, lin % sub_cols
        assert ((rs >= r0) & (rs < r0 + bh) & (cs >= c0) & (cs < c0 + bw)).all(), (case.name, k)
        assert r0 >= 0 and c0 >= 0 and r0 + bh <= sub_rows and c0 + bw <= sub_cols
        if b == 0 and d == 0:
            r = float(np.float32(case.circles[k, 2]) * np.float32(case.radius_scale))
            grow = 2 if case.mode == CC.HEIGHT else 2 + 2.0 ** -24 * max(UTM_REACH / abs(a), UTM_REACH / abs(e))
            assert bw <= 2 * (r * 1.0001 + 1e-3) / abs(a) + 2 * grow + 1 and bh <= 2 * (r * 1.0001 + 1e-3) / abs(e) + 2 * grow + 1


UTM_REACH = 5.32e6                               # no coordinate of any case's raster is larger


def test_f32_rounding_takes_in_rows_far_outside_the_circle():
    """NDVI mode: crowns with an oracle-inside pixel whose float64 position lies more than r + two pixels from the centre along y —
    at least a quarter of them at 0.02 m and a tenth at 0.05 m. The height-mode twins (float64 test) have none."""
    share = {}
    for case in CC.cases("f32_rounding"):
        masks, xs, ys, _ = CC.inside_masks(case)
        r = case.circles[:, 2].astype(np.float64) * case.radius_scale
        far = [bool((np.abs(ys[masks[k]] - float(case.circles[k, 1])) > r[k] + 2 * case.facts["pixel"]).any()) for k in range(len(r))]
        share[case.name] = float(np.mean(far))
        assert case.circles.shape[0] == 64 and ((r / case.facts["pixel"] >= 1.5) & (r / case.facts["pixel"] <= 30)).all()
        assert len(np.unique(case.raster)) == case.raster.size
    print(share)
    for name, s in share.items():
        if name.endswith("/height"):
            assert s == 0.0, (name, s)
        else:
            assert s >= (0.25 if "0.02m" in name else 0.10), (name, s)


def test_nan_pixels_hold_the_stated_number_of_nans():
    for case in CC.cases("nan_pixels"):
        masks, _, _, flat = CC.inside_masks(case)
        counts = [int(np.isnan(flat[masks[k]]).sum()) for k in range(len(CC.NAN_CROWNS))]
        assert counts == case.facts["nan_inside"]
        by = dict(zip(CC.NAN_CROWNS, range(len(CC.NAN_CROWNS))))
        assert counts[by["one"]] == 1 and counts[by["several"]] == 5 and counts[by["ring_outside"]] == 0
        assert counts[by["all"]] == int(masks[by["all"]].sum()) > 256
        assert np.isnan(flat[masks[by["first"]]][0]) and np.isnan(flat[masks[by["last"]]][-1])
        for what, on in (("stride", True), ("off_stride", False)):
            k = by[what]
            (lin,) = np.flatnonzero(masks[k] & np.isnan(flat))
            p = CC.box_position(case, k, int(lin))
            assert p > 0 and (p % 256 == 0) == on
        # the ring: NaNs in the crown's box, none inside the circle, and the nearest pixels outside it are among them
        k = by["ring_outside"]
        r0, c0, bh, bw = CC.kernel_box(case, k)
        box = case.raster[r0:r0 + bh, c0:c0 + bw]
        assert np.isnan(box).sum() == box.size - masks[k].sum() > 0


def test_ties_have_at_least_two_maxima_inside_every_crown():
    seen_first_zero = set()
    for case in CC.cases("ties"):
        masks, _, _, flat = CC.inside_masks(case)
        for k in range(case.circles.shape[0]):
            v = flat[masks[k]]
            assert v.size > 1024 and (v == v.max()).sum() >= 2, (case.name, k)
            if case.name.startswith("signed_zero"):
                zeros = v[v == 0]
                assert v.max() == 0 and {bool(np.signbit(z)) for z in zeros} == {False, True}
                seen_first_zero.add(bool(np.signbit(zeros[0])))
        if case.name.startswith("placed"):
            lins = [np.flatnonzero(masks[k]) for k in range(4)]
            hits = case.facts["placed"]
            for k in range(4):
                assert sorted(hits[k]) == [int(i) for i in np.flatnonzero(masks[k] & (flat == 9.0))] and flat[masks[k]].max() == 9.0
            assert hits[0][0] == lins[0][0] and hits[1] == [int(lins[1][-2]), int(lins[1][-1])]
            first, later = (CC.box_position(case, 2, h) for h in hits[2])
            assert first < later and first % 256 > later % 256                      # the later tie sits on a lower thread
            a, _, b = (CC.box_position(case, 3, h) for h in hits[3])
            assert b == a + 256
    assert seen_first_zero == {False, True}


def test_boundary_pixels_lie_on_the_circle_in_float32_and_float64():
    for case in CC.cases("boundary"):
        masks, xs, ys, flat = CC.inside_masks(case)
        cols = case.raster.shape[1]
        for marks, on in ((case.facts["on_circle"], True), (case.facts["just_outside"], False)):
            for k, (row, col) in marks.items():
                lin = row * cols + col
                cx, cy, r = case.circles[k]
                assert flat[lin] == 5.0 == case.raster.max()
                d64 = (xs[lin] - float(cx)) ** 2 + (ys[lin] - float(cy)) ** 2
                dx32, dy32 = np.float32(xs[lin]) - cx, np.float32(ys[lin]) - cy
                d32 = dx32 * dx32 + dy32 * dy32
                assert d32.dtype == np.float32
                if on:
                    assert d64 == float(r) ** 2 and d32 == r * r and masks[k][lin]
                else:
                    assert d64 == float(r) ** 2 + 1 and d32 == r * r + np.float32(1) and not masks[k][lin]
                    # no pixel outside the circle is nearer to it: integer geometry, so the next distance^2 after r^2 is r^2 + 1
        assert masks[4].sum() == 1 and masks[5].sum() == 0 and masks[6].sum() == 0


def test_clipping_orientation_windows_and_grid_cover_what_they_name():
    for case in CC.cases("clipping"):
        masks = CC.inside_masks(case)[0]
        n = masks.sum(axis=1)
        whole = 197                                      # lattice points within 8 pixels: what an unclipped r = 4 m circle holds
        assert (n[:8] > 0).all() and (n[:8] < whole).all() and (n[case.facts["empty"]] == 0).all()
        assert n[20] == case.raster.size and n[case.facts["single"]] == 1
        assert case.raster.shape in ((37, 301), (301, 37))
        # the quarter-metre-short circles still have a box on the raster; the far ones have none
        for k in range(8, 12):
            assert min(CC.kernel_box(case, k)[2:]) >= 1
        for k in range(12, 20):
            assert min(CC.kernel_box(case, k)[2:]) <= 0
    names = {c.name.split("/")[0] for c in CC.cases("orientation")}
    assert names == {"south_up", "west_positive", "south_up_west_positive", "rotated", "anisotropic"}
    for case in CC.cases("orientation"):
        a, b, _, d, e, _ = case.transform
        n = CC.inside_masks(case)[0].sum(axis=1)
        assert (n > 0).all() and case.raster.shape[0] <= 96 and case.raster.shape[1] <= 96
        assert (b != 0 and d != 0) == case.name.startswith("rotated")
    for case in CC.cases("windows"):
        r_lo, c_lo, sub_rows, sub_cols = CC.window(case)
        assert r_lo != c_lo and case.raster.shape[0] != case.raster.shape[1] and sub_rows * sub_cols < case.raster.size
        assert (sub_rows == 1) == case.name.startswith("one_row") and (sub_cols == 1) == case.name.startswith("one_column")
        n = CC.inside_masks(case)[0].sum(axis=1)
        assert (n[:-2] > 0).sum() >= 3 and (n[-2:] == 0).all()
    grid = {c.name: c for c in CC.cases("scale_and_grid")}
    assert {grid[f"scale{s}/ndvi"].radius_scale for s in (0.3, 0.7)} == {0.3, 0.7}
    for mode in ("height", "ndvi"):
        assert grid[f"one_crown/{mode}"].circles.shape[0] == 1 and grid[f"300_crowns/{mode}"].circles.shape[0] == 300
        dup = grid[f"duplicates/{mode}"]
        for g in dup.facts["groups"]:
            assert len(g) >= 2 and all(np.array_equal(dup.circles[g[0]], dup.circles[j]) for j in g)


def test_extremes_hold_what_they_name():
    by = {c.name: (c, CC.expected("extremes", i)) for i, c in enumerate(CC.cases("extremes"))}
    case, want = by["infinities/height"]
    assert np.isfinite(want[0, 0]) and want[1, 0] == np.inf and want[2, 0] == np.inf          # crown 0 holds the -inf only
    want = by["infinities/ndvi"][1]
    assert want[0, 0] == -np.inf and np.isfinite(want[0, 1]) and want[0, 2] == -np.inf and np.isnan(want[0, 3])
    assert want[1, 1] == np.inf and want[1, 2] == np.inf and np.isnan(want[2, 2]) and (want[2, 0], want[2, 1]) == (-np.inf, np.inf)
    case, want = by["all_minus_inf/height"]
    xs, ys = CC.inside_masks(case)[1:3]
    for k in range(case.circles.shape[0]):
        first = int(np.flatnonzero(CC.inside_masks(case)[0][k])[0])
        assert want[k].tolist() == [-np.inf, np.float32(xs[first]), np.float32(ys[first])]
    want = by["all_minus_inf/ndvi"][1]
    assert (want[:, :3] == -np.inf).all() and np.isnan(want[:, 3]).all()
    case = by["denormals/height"][0]
    assert (case.raster > 0).all() and (case.raster < np.finfo(np.float32).tiny).all() and np.unique(case.raster).size == case.raster.size
    case, want = by["constant/ndvi"]
    v = np.float32(case.facts["constant"])
    assert np.array_equal(want, np.tile(np.array([v, v, v, 0], np.float32), (want.shape[0], 1)))
    case, want = by["large_mean_tiny_spread/ndvi"]
    assert (want[:, 2] > 1000).all() and (want[:, 3] > 0).all() and (want[:, 3] < 1e-4).all()
