"""crown_device.sparse_rows under its two callers, on tiny inputs: box_pairs.box_pairs_ab (td_box_pairs_ab_count / _fill) against
its host twin and a list pinned by hand, at and one below the cap and with no pair at all; box_pairs.connected_pairs_device
(td_crown_pairs_count / _fill) against the dense mask of postprocessing.filter_polygons_by_iou_and_area's formula."""
import numpy as np
import pytest

from treedetection_amd import box_pairs as BP

pytestmark = pytest.mark.gpu

NAN = float("nan")
# overlapping, touching (A0 and B1 share the line x = 2), disjoint, and one NaN box on each side
BOXES_A = np.array([[0, 0, 2, 2], [1, 1, 3, 3], [10, 10, 12, 12], [NAN, 0, 2, 2], [4, 0, 6, 2]], dtype=np.float64)
BOXES_B = np.array([[1, 1, 2.5, 2.5], [2, 0, 4.5, 2], [5, 1, 11, 11], [0, 0, NAN, 1]], dtype=np.float64)
PAIRS = [[0, 0], [1, 0], [1, 1], [2, 2], [4, 1], [4, 2]]       # (A0, B1) only touch; A3 and B3 pair with nothing


def same_pairs(got, want):
    return got.dtype == np.int32 and got.shape == (len(want), 2) and got.tolist() == want


def test_the_host_twin_finds_the_pinned_pairs():
    assert same_pairs(BP.box_pairs_ab(BOXES_A, BOXES_B, device=None), PAIRS)


def test_box_pairs_ab_equals_the_host_twin(capsys):
    assert same_pairs(BP.box_pairs_ab(BOXES_A, BOXES_B, device=0), PAIRS)
    assert capsys.readouterr().out == ""


def test_box_pairs_ab_at_and_below_the_cap(monkeypatch, capsys):
    monkeypatch.setattr(BP, "MAX_DEVICE_PAIRS", 6)
    assert same_pairs(BP.box_pairs_ab(BOXES_A, BOXES_B, device=0), PAIRS)
    assert capsys.readouterr().out == ""                        # six pairs are stored by the device path
    monkeypatch.setattr(BP, "MAX_DEVICE_PAIRS", 5)
    assert same_pairs(BP.box_pairs_ab(BOXES_A, BOXES_B, device=0), PAIRS)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "more than 5 candidate pairs" in out and "using the host function" in out


def test_box_pairs_ab_without_a_pair():
    a = np.array([[0, 0, 1, 1], [2, 0, 3, 1], [4, 0, 5, 1]], dtype=np.float64)
    b = a + np.array([0, 5, 0, 5.0])
    for device in (0, None):
        got = BP.box_pairs_ab(a, b, device=device)
        assert got.dtype == np.int32 and got.shape == (0, 2)


def test_connected_pairs_device_equals_the_dense_mask():
    bb = np.array([[0, 0, 4, 4], [0.5, 0, 4.5, 4], [0, 0, 4, 2.2], [0, 0, 4, 3.9]], dtype=np.float32)
    ar = np.array([16, 15, 8.8, 2], dtype=np.float16)
    iou_thr, area_thr = np.float32(0.5), np.float16(0.5)
    # filter_polygons_by_iou_and_area's mask: float32 boxes, float16 areas
    x_a, y_a = np.maximum(bb[:, 0][:, None], bb[:, 0]), np.maximum(bb[:, 1][:, None], bb[:, 1])
    x_b, y_b = np.minimum(bb[:, 2][:, None], bb[:, 2]), np.minimum(bb[:, 3][:, None], bb[:, 3])
    inter = np.maximum(0, x_b - x_a) * np.maximum(0, y_b - y_a)
    area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    iou = inter / (area[:, None] + area - inter)
    mask = (iou > iou_thr) & (np.abs(ar[:, None] - ar) / np.maximum(ar[:, None], ar) < area_thr)
    np.fill_diagonal(mask, False)
    assert mask.tolist() == [[False, True, True, False], [True, False, False, False], [True, False, False, False], [False] * 4]
    assert (iou > iou_thr)[3, :3].all()                         # box 3 is kept out by its area alone
    row_start, cols = BP.connected_pairs_device(bb, ar, iou_thr, area_thr)
    assert row_start.dtype == np.int64 and cols.dtype == np.int32 and row_start.tolist() == [0, 2, 3, 4, 4]
    assert [sorted(cols[row_start[i]:row_start[i + 1]].tolist()) for i in range(4)] == [list(np.flatnonzero(r)) for r in mask]
    row_start, cols = BP.connected_pairs_device(bb[:1], ar[:1], iou_thr, area_thr)
    assert row_start.tolist() == [0, 0] and cols.dtype == np.int32 and cols.shape == (0,)
