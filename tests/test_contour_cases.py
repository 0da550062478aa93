"""CPU proof that tests/contour_cases.py holds what tests/test_contours_limits_gpu.py claims to feed the device tracer: every
case has the label-image size, the contour count and the nesting depth its name states (literal expectations below, checked
with the oracle), the product's host tracer agrees with the oracle on it point for point, its expected status follows
from those numbers by the rule of include/treedet.h, and the word / window family puts outer and hole starts on the columns
around the 32-bit word and the 64-pixel window. Then the controls of the GPU checker: a correct result built on the CPU
passes ``check_outputs`` and every perturbed copy of it is rejected."""
import numpy as np
import pytest

from tests import contour_cases as cc
from treedetection_amd.contours import find_contours as host_find_contours

# name, w, h, (w+2)*(h+2), contours, tree levels, status
SIZE = [("blob-94x62", 94, 62, 6144, 2, 2, 0), ("blob-62x94", 62, 94, 6144, 2, 2, 0), ("blob-73x80", 73, 80, 6150, 2, 2, 0),
        ("blob-1x2047", 1, 2047, 6147, 2, 1, 0), ("blob-3x1227", 3, 1227, 6145, 2, 2, 0), ("blob-126x222", 126, 222, 28672, 2, 2, 0),
        ("blob-51x539", 51, 539, 28673, 2, 2, 1), ("blob-176x160", 176, 160, 28836, 2, 2, 1),
        ("ones-94x62", 94, 62, 6144, 1, 1, 0), ("ones-126x222", 126, 222, 28672, 1, 1, 0)]
COUNT = [("iso-256", 63, 15, 1105, 256, 1, 0), ("iso-257", 63, 17, 1235, 257, 1, 2), ("rings-128", 63, 31, 2145, 256, 2, 0),
         ("rings-128-plus-1", 65, 31, 2211, 257, 2, 2), ("iso-65", 63, 5, 455, 65, 1, 0), ("iso-129", 63, 9, 715, 129, 1, 0),
         ("iso-256-late-257th", 63, 19, 1365, 257, 1, 2)]
NEST = [("rings-18", 73, 73, 5625, 37, 37, 0), ("rings-30", 121, 121, 15129, 61, 61, 0), ("twin-stacks", 39, 21, 943, 20, 11, 0),
        ("three-islands", 24, 14, 416, 8, 4, 0), ("diagonal-line", 20, 20, 484, 1, 1, 0), ("staircase", 16, 16, 324, 1, 1, 0),
        ("diamond", 13, 13, 225, 37, 2, 0)]
DEGENERATE = [("1x1", 1, 1, 9, 1, 1, 0), ("row-70", 70, 1, 216, 1, 1, 0), ("column-70", 1, 70, 216, 1, 1, 0), ("empty-4x4", 4, 4, 36, 0, 0, 0),
              ("empty-5x130", 130, 5, 924, 0, 0, 0), ("zero-width", 0, 4, 12, 0, 0, 0), ("negative-width", 0, 4, 12, 0, 0, 0),
              ("zero-height", 4, 0, 12, 0, 0, 0)]
WIDTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129)
STRIPES = {31: 16, 32: 16, 33: 17, 63: 32, 64: 32, 65: 33, 127: 64, 128: 64, 129: 65}
# contours and tree levels of each content of the word / window family
WORD_CONTENT = {"ones": (1, 1), "last": (1, 1), "first": (1, 1), "bars": (2, 1), "bridge": (2, 2), "comb": (7, 1), "ladder": (11, 3), "rings": (4, 4)}


def _word_table():
    rows = []
    for w in WIDTHS:
        rows += [(f"w{w}-{k}", w, 5, (w + 2) * 7, *WORD_CONTENT[k], 0) for k in ("ones", "last", "first")]
        rows.append((f"w{w}-stripes", w, 5, (w + 2) * 7, STRIPES[w], 1, 0))
        for a in (31, 32, 33, 63, 64, 65):
            if w >= a + 3:
                if a in (31, 63, 64):
                    rows.append((f"w{w}-bars-{a}|{a + 1}", w, 5, (w + 2) * 7, 2, 1, 0))
                rows.append((f"w{w}-bridge-{a}|{a + 1}", w, 5, (w + 2) * 7, 2, 2, 0))
    for w in (64, 65):
        rows += [(f"w{w}-{k}", w, 5, (w + 2) * 7, *WORD_CONTENT[k], 0) for k in ("comb", "ladder")]
    rows += [("w129-ladder-60", 129, 5, 917, 9, 3, 0), ("w129-ladder-63", 129, 5, 917, 9, 3, 0)]
    rows.append(("w130-rings", 130, 9, 1452, 4, 4, 0))
    return rows


TABLES = {"size": SIZE, "word": _word_table(), "count": COUNT, "nest": NEST, "degenerate": DEGENERATE}
ROWS = [(f, *r) for f, rows in TABLES.items() for r in rows]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_case_list_is_the_stated_one():
    assert len(TABLES["word"]) == 82 and len(ROWS) == 114
    for f, rows in TABLES.items():
        assert [c.name for c in cc.family(f)] == [r[0] for r in rows], f
    names = [r[1] for r in ROWS]
    assert len(set(names)) == len(names)
    assert cc.SIZE_TABLE == [(r[3], r[1], r[2], r[6]) for r in SIZE[:8]]
    assert (cc.CMAX, cc.LABEL_SMALL, cc.LABEL_LARGE) == (256, 6144, 28672)


@pytest.mark.parametrize("fam,name,w,h,elems,count,levels,status", ROWS, ids=[r[1] for r in ROWS])
def test_case_is_what_its_name_says(fam, name, w, h, elems, count, levels, status):
    c = cc.case(name)
    assert c.mask.dtype == bool and c.mask.shape == (h, w) and cc.need(c.mask) == elems and elems <= 29000
    want = cc.contours_of(c.mask)
    depth = cc.tree_depths(want)
    assert len(want) == count and (max(depth) + 1 if depth else 0) == levels
    if c.mask.size:
        assert _same(host_find_contours(c.mask.astype(np.uint8)), want)
    else:
        assert want == []
    assert status == cc.status_rule(elems, count) == c.status          # the rule, from the numbers above; then the case's claim


def test_size_family_touches_every_edge_and_sits_on_both_seams():
    for c in cc.family("size"):
        m = c.mask
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any(), c.name
    elems = sorted({r[3] for r in SIZE})
    assert elems == [6144, 6145, 6147, 6150, 28672, 28673, 28836]
    assert cc.LABEL_SMALL in elems and cc.LABEL_SMALL + 1 in elems and cc.LABEL_LARGE in elems and cc.LABEL_LARGE + 1 in elems
    for name in ("ones-94x62", "ones-126x222"):
        m = cc.case(name).mask
        h, w = m.shape
        assert [c.tolist() for c in cc.contours_of(m)] == [[[0, 0], [0, h - 1], [w - 1, h - 1], [w - 1, 0]]]
    # run in reversed order on the same det_info, no position may expect the row the first run left there
    rows = [(r[6], r[4] if r[6] == 0 else 0, sum(len(x) for x in cc.contours_of(cc.case(r[0]).mask)) if r[6] == 0 else 0) for r in SIZE]
    assert len(rows) % 2 == 0 and all(a != b for a, b in zip(rows, rows[::-1]))


def _starts(case):
    """(column, is_hole) of every border start: the first point of a contour is its start pixel, odd tree depth = hole."""
    cs = cc.contours_of(case.mask)
    return [(int(c[0][0]), d % 2 == 1) for c, d in zip(cs, cc.tree_depths(cs))]


def test_word_family_starts_borders_on_the_word_and_window_columns():
    outer, hole = set(), set()
    for c in cc.family("word"):
        for col, is_hole in _starts(c):
            (hole if is_hole else outer).add(col)
    for col in (31, 32, 33, 63, 64, 65):
        assert col in outer and col in hole, col
    assert 0 in outer and 0 in hole and 128 in outer
    # the single pixels are where their names say, the bars' second outer border starts two past the first bar's end
    for w in WIDTHS:
        assert _starts(cc.case(f"w{w}-last")) == [(w - 1, False)] and _starts(cc.case(f"w{w}-first")) == [(0, False)]
    assert sorted(_starts(cc.case("w129-bars-63|64"))) == [(0, False), (65, False)]
    assert sorted(_starts(cc.case("w129-bridge-63|64"))) == [(0, False), (63, True)]
    assert sorted(_starts(cc.case("w130-rings"))) == [(0, False), (0, True), (65, False), (65, True)]


def test_comb_and_ladder_put_marked_pixels_where_the_scan_must_read_them():
    """After the outer border is followed from row 0 every tooth pixel is marked (f != 1). Rows 1-4 then hold: a marked pixel
    before the first candidate of the row's first window (tooth 5 before the pixels at 7 / 10), a row without any candidate
    (row 1 and 3), and a marked pixel in column 63 = lane 63 of that row's only full window."""
    for w in (64, 65):
        m = cc.case(f"w{w}-comb").mask
        assert m[0].all() and m[1:, 63].all() and m[1:, 5].all()
        for r in (1, 3):
            assert set(np.flatnonzero(m[r]).tolist()) == {5, 20, 41, 63}           # only teeth: no candidate in these rows
        assert np.flatnonzero(m[2]).tolist()[:2] == [5, 10] and np.flatnonzero(m[4]).tolist()[:2] == [5, 7]
        cs = cc.contours_of(m)
        assert [len(c) for c in cs].count(1) == 6 and len(cs) == 7
    for name, (w, rungs, pixels) in cc.LADDERS.items():
        lad = cc.case(name).mask
        assert sorted(np.flatnonzero(lad[2] & lad[1]).tolist()) == list(rungs) and lad.shape == (5, w)
        cs = cc.contours_of(lad)
        d = cc.tree_depths(cs)
        assert d.count(0) == 1 and d.count(1) == len(rungs) - 1 and d.count(2) == len(pixels)
        # every pixel hangs under the hole of ITS cell: the last hole before it in pre-order is that hole
        for i, c in enumerate(cs):
            if d[i] == 2:
                j = max(k for k in range(i) if d[k] == 1)
                left = int(cs[j][0][0])                                            # a hole starts on the rung left of its cell
                assert left in rungs and left < int(c[0][0]) < rungs[rungs.index(left) + 1]
    # row 2 of the wide ladders: the first window (columns 0-63) holds rung marks only, the last of them at column 60 / 63 (lane
    # 63), and the first pixel opens the second window as lane 0 / lane 1; two rung marks (100, 105) precede the second pixel
    for a, first in ((60, 64), (63, 65)):
        row = np.flatnonzero(cc.case(f"w129-ladder-{a}").mask[2]).tolist()
        assert row == [0, 20, 40, a, first, 100, 105, 110, 128]


def test_nesting_orders_most_recent_sibling_first():
    cs = cc.contours_of(cc.case("three-islands").mask)
    d = cc.tree_depths(cs)
    assert d == [0, 1, 2, 3, 2, 3, 2, 3]
    assert [c[0].tolist() for c, k in zip(cs, d) if k == 2] == [[15, 6], [8, 3], [2, 2]]      # found last, listed first
    cs = cc.contours_of(cc.case("twin-stacks").mask)
    d = cc.tree_depths(cs)
    assert d == [0, 1] + list(range(2, 11)) * 2 and cs[2][0].tolist() == [20, 2] and cs[11][0].tolist() == [2, 2]
    assert cc.tree_depths(cc.contours_of(cc.case("rings-18").mask)) == list(range(37))
    cs = cc.contours_of(cc.case("diamond").mask)
    assert cc.tree_depths(cs) == [0] + [1] * 36 and all(len(c) == 4 for c in cs[1:])
    line = cc.contours_of(cc.case("diagonal-line").mask)
    assert [c.tolist() for c in line] == [[[0, 0], [19, 19]]]


# ---- controls of the GPU checker -------------------------------------------------------------------------------------------
def _control_batch():
    names = ["three-islands", "w65-ladder", "iso-257", "empty-4x4", "blob-51x539", "iso-65"]
    images = [cc.dets_of([cc.case(n) for n in names], seed=1), cc.dets_of([cc.case("diamond")], seed=2), []]
    images[1] = images[1] + [cc.Det(3, 4, np.ones((6, 6), bool), 0)]          # behind the count: must not be traced
    counts = [6, 1, 0]
    return images, counts, 6, 700


def test_checker_accepts_a_correct_result():
    images, counts, Dn, cap = _control_batch()
    out = cc.expected_outputs(images, counts, Dn, cap)
    assert cc.check_outputs(out, images, counts, cap) == {0: 5, 1: 1, 2: 1, 4: 0}
    assert out["det_info"][0, :, 0].tolist() == [0, 0, 2, 0, 1, 0] and (out["det_info"][1, 1:] == 0).all()
    # a full point buffer: the block that does not fit is flagged, and only where the test says so
    total = sum(len(c) for c in cc.contours_of(cc.case("diamond").mask))
    two = [[cc.Det(0, 0, cc.case("diamond").mask, 0)] * 2]
    out = cc.expected_outputs(two, [2], 2, 2 * total - 1)
    assert out["det_info"][0].tolist() == [[0, 37, 0, total], [4, 0, total, 0]] and out["img_pts"][0] == 2 * total
    assert cc.check_outputs(out, two, [2], 2 * total - 1, full={0: 1})[4] == 1
    with pytest.raises(AssertionError, match="status 4"):
        cc.check_outputs(out, two, [2], 2 * total - 1)
    assert cc.check_outputs(cc.expected_outputs(two, [2], 2, 2 * total), two, [2], 2 * total) == {0: 2, 1: 0, 2: 0, 4: 0}


def _swap_contours(o):
    o["cont_info"][0, 0, [1, 2]] = o["cont_info"][0, 0, [2, 1]]


def _point_off_by_one(o):
    o["pts"][0, int(o["det_info"][0, 1, 2]) + 3, 0] += 1


def _status_to_two(o):
    o["det_info"][0, 5, 0] = 2


def _status_two_with_contents_cleared(o):
    o["det_info"][0, 5] = (2, 0, 0, 0)


def _canary_behind_block(o):
    o["pts"][0, int(o["img_pts"][0]), 1] = 0


def _canary_in_next_image(o):
    o["pts"][1, int(o["img_pts"][1]) + 5, 0] = 17


def _cont_info_past_nc(o):
    o["cont_info"][0, 0, 8, 1] = 4


def _cont_info_of_flagged(o):
    o["cont_info"][0, 2, 0] = (0, 1)


def _stale_row_never_written(o):
    o["det_info"][0, 4] = cc.INFO_CANARY


def _stale_row_from_previous_batch(o):
    o["det_info"][0, 4] = (0, 2, 0, 240)


def _stale_row_behind_count(o):
    o["det_info"][1, 1] = (0, 1, 0, 4)


def _traced_behind_count(o):
    o["cont_info"][1, 1, 0] = (0, 4)


def _flagged_too_eagerly(o):
    o["det_info"][0, 0] = (2, 0, 0, 0)


def _image_points_off(o):
    o["img_pts"][0] += 1


@pytest.mark.parametrize("damage", [_swap_contours, _point_off_by_one, _status_to_two, _status_two_with_contents_cleared, _canary_behind_block,
                                    _canary_in_next_image, _cont_info_past_nc, _cont_info_of_flagged, _stale_row_never_written,
                                    _stale_row_from_previous_batch, _stale_row_behind_count, _traced_behind_count, _flagged_too_eagerly,
                                    _image_points_off], ids=lambda f: f.__name__.lstrip("_"))
def test_checker_rejects(damage):
    images, counts, Dn, cap = _control_batch()
    out = cc.expected_outputs(images, counts, Dn, cap)
    before = {k: v.copy() for k, v in out.items()}
    damage(out)
    assert any(not np.array_equal(out[k], before[k]) for k in out)
    with pytest.raises(AssertionError):
        cc.check_outputs(out, images, counts, cap)


def test_checker_rejects_two_detections_sharing_one_block():
    m = cc.case("diamond").mask
    total = sum(len(c) for c in cc.contours_of(m))
    two = [[cc.Det(7, 9, m, 0)] * 2]
    out = cc.expected_outputs(two, [2], 2, 400)
    cc.check_outputs(out, two, [2], 400)
    out["det_info"][0, 1, 2] = 0                                   # same points, same block: every point still reads right
    out["pts"][0, total: 2 * total] = cc.PTS_CANARY
    with pytest.raises(AssertionError, match="overlap"):
        cc.check_outputs(out, two, [2], 400)
