"""The device side of treedetection_amd.evaluation: td_box_pairs_ab_count / td_box_pairs_ab_fill (boxpairs_ab.hip) against the host
twin td_box_pairs_ab as sorted sets, at the smallest shapes where the kernel can go wrong (one box, a ragged second row block, a
ragged second column chunk, rows of very different lengths, NaN and touching boxes), and evaluate(device=0) against
evaluate(device=None) bit for bit. The host twin is held to a brute force in tests/test_evaluation.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cases as E  # noqa: E402
from treedetection_amd import _lib  # noqa: E402
from treedetection_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu


def device_rows(a, b):
    """The two raw calls with the prefix sum in between → (counts, row_start, cols); cols is filled with -1 beforehand."""
    import torch
    lib = _lib.load()
    d_a, d_b = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    n_a, n_b = len(a), len(b)
    counts = torch.full((n_a,), 123, dtype=torch.int32, device="cuda")          # (the call zeroes it)
    _lib.check(lib.td_box_pairs_ab_count(d_a.data_ptr(), n_a, d_b.data_ptr(), n_b, counts.data_ptr(), _lib.stream_ptr()), "count")
    row_start = torch.zeros(n_a + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(counts, 0, dtype=torch.int64, out=row_start[1:])
    total = int(row_start[-1].item())
    cols = torch.full((total + 1,), -1, dtype=torch.int32, device="cuda")       # one slot more than the rows hold: it stays -1
    cursor = torch.full((n_a,), 99, dtype=torch.int32, device="cuda")
    _lib.check(lib.td_box_pairs_ab_fill(d_a.data_ptr(), n_a, d_b.data_ptr(), n_b, row_start.data_ptr(), cursor.data_ptr(), cols.data_ptr(),
                                        _lib.stream_ptr()), "fill")
    torch.cuda.synchronize()
    assert torch.equal(cursor, counts)                                          # every row's cursor ends at its count
    return counts.cpu().numpy(), row_start.cpu().numpy(), cols.cpu().numpy()


def check_against_host(a, b):
    want = EV.box_pairs_ab(a, b, device=None)
    counts, row_start, cols = device_rows(a, b)
    total = int(row_start[-1])
    assert total == len(want) and np.array_equal(counts, np.bincount(want[:, 0], minlength=len(a)))        # counts = row lengths
    assert cols[total] == -1 and (cols[:total] >= 0).all()                                                   # every slot written, none beyond
    got = np.stack([np.repeat(np.arange(len(a)), counts), cols[:total]], axis=1)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert np.array_equal(got, want)                          # the same set: no duplicate within a row, so each slot was written once
    assert np.array_equal(EV.box_pairs_ab(a, b, device=0), want)
    return want


@pytest.mark.parametrize("name", ["1x1", "257x1025", "1025x257", "nan_slots", "touching_edge", "touching_corner", "a_hair_inside", "zero_width",
                                  "inverted", "infinite", "identical", "utm_far_apart"])
def test_device_pairs_equal_the_host_twin(name):
    a, b = E.box_cases()[name]
    want = check_against_host(a, b)
    assert np.array_equal(want, E.brute_pairs(a, b))
    if name in ("257x1025", "1025x257"):
        assert len(want) > 1025


def test_heavy_overlap_3000_by_2100():
    a, b = E.heavy_overlap()
    want = check_against_host(a, b)
    per_row = np.bincount(want[:, 0], minlength=len(a))
    assert len(want) > 100_000 and per_row.max() > 4 * max(per_row.min(), 1)


def test_empty_sets_launch_nothing_and_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = _lib.load()
    some = E.box_cases()["1x5"][1]
    assert EV.box_pairs_ab(np.zeros((0, 4)), some, device=0).shape == (0, 2) and EV.box_pairs_ab(some, [], device=0).shape == (0, 2)
    boxes = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
    counts = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    rows = torch.zeros(9, dtype=torch.int64, device="cuda")
    cols = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    s = _lib.stream_ptr()
    count_args = [boxes.data_ptr(), 4, boxes.data_ptr(), 4, counts.data_ptr(), s]
    fill_args = [boxes.data_ptr(), 4, boxes.data_ptr(), 4, rows.data_ptr(), counts.data_ptr(), cols.data_ptr(), s]
    for fn, args, pointers in ((lib.td_box_pairs_ab_count, count_args, (0, 2, 4)), (lib.td_box_pairs_ab_fill, fill_args, (0, 2, 4, 5, 6))):
        for k in pointers:
            bad = list(args)
            bad[k] = None
            assert fn(*bad) == _lib.ERR_INVALID and b"null" in lib.td_last_error()
        for k in (0, 2):
            bad = list(args)
            bad[k] = boxes.data_ptr() + 8
            assert fn(*bad) == _lib.ERR_INVALID and b"aligned" in lib.td_last_error()
        for k in (1, 3):
            for count in (0, -1, 65535 * 1024 + 1):
                bad = list(args)
                bad[k] = count
                assert fn(*bad) == _lib.ERR_INVALID and b"n_a" in lib.td_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [7] * 8 and cols.tolist() == [7] * 8          # nothing ran


def same_records(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            if isinstance(w[key], np.ndarray):
                assert g[key].dtype == w[key].dtype and np.array_equal(g[key], w[key]), key
            elif isinstance(w[key], float):
                assert np.float64(g[key]).view(np.uint64) == np.float64(w[key]).view(np.uint64), (key, g[key], w[key])
            else:
                assert g[key] == w[key], key


def test_evaluate_on_the_device_equals_the_host_path_bit_for_bit():
    """About 400 seeded blob crowns against shifted, rescaled and partly deleted copies, one ring pair above the area kernel's
    vertex cap: the same matrix, hence the same records in every field."""
    pred, scores, ann = E.blob_scene()
    h_rows, h_cols, h_iou = EV.crown_iou_matrix(pred, ann, device=None)
    d_rows, d_cols, d_iou = EV.crown_iou_matrix(pred, ann, device=0)
    assert np.array_equal(h_rows, d_rows) and np.array_equal(h_cols, d_cols) and np.array_equal(h_iou.view(np.uint64), d_iou.view(np.uint64))
    assert len(h_cols) > len(pred) and h_rows[-1] - h_rows[-2] == 1 and h_cols[-1] == len(ann) - 1          # the capped pair is in it
    assert len(pred[-1]) + len(ann[-1]) - 2 > _lib.RING_PAIR_CAP
    iou_thresholds = (0.3, 0.5, 0.7)
    want = EV.evaluate(pred, scores, ann, iou_thresholds=iou_thresholds, device=None)
    got = EV.evaluate(pred, scores, ann, iou_thresholds=iou_thresholds, device=0)
    same_records(got, want)
    assert len(want) == 21 and 0 < want[0]["tp"] < len(ann) and want[0]["fp"] > 0 and want[0]["fn"] > 0
    assert want[0]["tp"] > want[14]["tp"] and want[0]["tp"] > want[6]["tp"]          # stricter thresholds match fewer
