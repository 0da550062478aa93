"""td_trace_contours_dev at its size, word, window and count limits: the crafted masks of tests/contour_cases.py (proved on the
CPU by tests/test_contour_cases.py) through the kernel, judged by the one strict checker ``contour_cases.check_outputs`` —
the status every detection must get, the oracle's contours in RETR_TREE order for the traced ones, and canaries around
everything the kernel may not write. All comparisons are exact."""
import inspect

import numpy as np
import pytest
import torch

from tests import contour_cases as cc
from treedetection_amd import _lib
from treedetection_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _upload(images, Dn, counts):
    region, offset, bits = cc.pack(images, Dn)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    return {"region": dev(region), "offset": dev(offset), "bits": dev(bits.view(np.int32)), "counts": dev(np.asarray(counts, np.int32)),
            "host": (region, offset, bits)}


def _buffers(B, Dn, pts_cap):
    return {k: torch.from_numpy(v).cuda() for k, v in cc.canary_outputs(B, Dn, pts_cap).items()}


def _launch(inp, buf):
    B, Dn = buf["det_info"].shape[:2]
    lib = _lib.load()
    _lib.check(lib.td_trace_contours_dev(inp["region"].data_ptr(), inp["offset"].data_ptr(), inp["bits"].data_ptr(), inp["bits"].shape[1],
                                         inp["counts"].data_ptr(), B, Dn, buf["pts"].data_ptr(), buf["pts"].shape[1], buf["img_pts"].data_ptr(),
                                         buf["det_info"].data_ptr(), buf["cont_info"].data_ptr(), _lib.stream_ptr()), "td_trace_contours_dev")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}


def _run(images, Dn, pts_cap, counts=None, full=None):
    counts = [len(d) for d in images] if counts is None else counts
    out = _launch(_upload(images, Dn, counts), _buffers(len(images), Dn, pts_cap))
    return out, cc.check_outputs(out, images, counts, pts_cap, full=full)


@pytest.mark.parametrize("fam,seen", [("size", {0: 8, 1: 2, 2: 0, 4: 0}), ("word", {0: 82, 1: 0, 2: 0, 4: 0}), ("count", {0: 4, 1: 0, 2: 3, 4: 0}),
                                      ("nest", {0: 7, 1: 0, 2: 0, 4: 0}), ("degenerate", {0: 8, 1: 0, 2: 0, 4: 0})])
def test_family_in_one_launch(fam, seen):
    cases = cc.family(fam)
    out, got = _run([cc.dets_of(cases, seed=len(cases))], Dn=len(cases), pts_cap=4096)
    print(fam, got)
    assert got == seen
    if fam == "degenerate":
        void = [i for i, c in enumerate(cases) if c.mask.size == 0]
        assert len(void) == 3 and (out["det_info"][0, void] == 0).all()


def test_size_classes_twice_on_the_same_det_info():
    """Both seams, then the same cases in reversed order without refilling det_info: a detection that neither launch
    claims keeps the other case's row from the first run (tests/test_contour_cases.py: no position expects it)."""
    cases = cc.family("size")
    Dn, cap = len(cases), 2048
    first = [cc.dets_of(cases, seed=5)]
    second = [first[0][::-1]]
    buf = _buffers(1, Dn, cap)
    out = _launch(_upload(first, Dn, [Dn]), buf)
    cc.check_outputs(out, first, [Dn], cap)
    fresh = cc.canary_outputs(1, Dn, cap)
    buf["pts"].copy_(torch.from_numpy(fresh["pts"]))
    buf["cont_info"].copy_(torch.from_numpy(fresh["cont_info"]))
    out2 = _launch(_upload(second, Dn, [Dn]), buf)
    cc.check_outputs(out2, second, [Dn], cap)
    assert out2["det_info"][0, :, 0].tolist() == out["det_info"][0, ::-1, 0].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]


def test_point_buffer_exact_fit_and_one_short():
    m = cc.case("three-islands").mask
    total = sum(len(c) for c in cc.contours_of(m))
    images = [[cc.Det(11, 7, m, 0), cc.Det(400, 300, m, 0)], [], [cc.Det(5, 5, cc.case("w65-ladder").mask, 0)]]
    out, seen = _run(images, Dn=2, pts_cap=2 * total)
    assert seen == {0: 3, 1: 0, 2: 0, 4: 0} and out["img_pts"].tolist() == [2 * total, 0, 42]
    out, seen = _run(images, Dn=2, pts_cap=2 * total - 1, full={0: 1})      # either copy may lose: the atomic decides
    assert seen == {0: 2, 1: 0, 2: 0, 4: 1}
    assert sorted(out["det_info"][0].tolist()) == [[0, 8, 0, total], [4, 0, total, 0]] and out["img_pts"][0] == 2 * total
    assert (out["pts"][1] == cc.PTS_CANARY).all()


def test_production_batch_shape():
    B, Dn, counts = 8, 100, [0, 1, 100, 37, 100, 64, 65, 2]
    pts_cap = inspect.signature(Engine.alloc_contours).parameters["points_cap"].default      # as Engine sizes its buffers
    assert Engine.CONTOUR_MAX == cc.CMAX and isinstance(pts_cap, int)
    pool = [c for f in cc.FAMILIES for c in cc.family(f) if c.status == 0]
    assert len(pool) == 109
    rng = np.random.default_rng(8)
    images, k = [], 0
    for b in range(B):
        dets = cc.dets_of([pool[(k + i) % len(pool)] for i in range(counts[b])], seed=b)
        k += counts[b]
        # behind the count: a valid region over garbage bits, which must not be traced
        dets += [cc.Det(int(rng.integers(0, 900)), int(rng.integers(0, 900)), rng.random((int(rng.integers(1, 40)), int(rng.integers(1, 70)))) < 0.5, 0)
                 for _ in range(Dn - counts[b])]
        images.append(dets)
    out, seen = _run(images, Dn=Dn, pts_cap=pts_cap, counts=counts)
    assert seen == {0: sum(counts), 1: 0, 2: 0, 4: 0} and out["img_pts"][0] == 0 and (out["pts"][0] == cc.PTS_CANARY).all()


def test_flagged_detections_fall_back_to_the_host_tracer():
    from treedetection_amd.contours import tile_polygons_json, tile_polygons_json_dev
    cases = [cc.case("blob-51x539"), cc.case("iso-257"), cc.case("rings-18")]
    images = [cc.dets_of(cases, seed=3)]
    inp = _upload(images, 3, [3])
    out = _launch(inp, _buffers(1, 3, 1024))
    assert cc.check_outputs(out, images, [3], 1024) == {0: 1, 1: 1, 2: 1, 4: 0}
    assert out["det_info"][0, :, 0].tolist() == [1, 2, 0]
    region, offset, bits = inp["host"]
    scores = np.array([0.9, 0.8, 0.7], np.float32)
    classes = np.zeros(3, np.int32)
    t = (0.2, 0.0, 412000.0, 0.0, -0.2, 5319000.0)
    want = tile_polygons_json(region[0], offset[0], bits[0].view(np.int32), scores, classes, t, "img.tif")
    args = (out["pts"][0], out["det_info"][0], out["cont_info"][0], region[0], offset[0])
    assert tile_polygons_json_dev(*args, None, scores, classes, t, "img.tif") is None
    got = tile_polygons_json_dev(*args, bits[0].view(np.int32), scores, classes, t, "img.tif")
    assert got == want and len(want) > 2
