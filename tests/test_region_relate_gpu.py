"""td_region_relate_dev (regionrelate.hip: a wave per query ring) against the host td_region_relate on the crafted families of
tests/region_cases.py, which tests/test_region_cases.py proves against the exact oracle: the flags are equal query for query, and
the kernel decides everything itself except the queries built beyond one of its fixed capacities."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import region_cases as RC  # noqa: E402
from treedetection_amd import _lib, vector  # noqa: E402
from treedetection_amd.vector import Region  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILIES = RC.families()


@pytest.mark.parametrize("fam", FAMILIES, ids=[f["name"] for f in FAMILIES])
def test_family_equals_the_host_function(fam):
    r = Region(fam["forest"])
    hi, hw = r.relate(fam["queries"])
    di, dw = r.relate(fam["queries"], device=0)
    print(fam["name"], "deferred", r.last_deferred_queries.tolist())
    assert di.tolist() == hi.tolist() and dw.tolist() == hw.tolist()
    if fam["want"] is not None:
        assert list(zip(di.tolist(), dw.tolist())) == fam["want"]
    # exactly the queries built beyond a capacity were left to the host function (and merged right, above)
    assert r.last_deferred_queries.tolist() == fam["beyond"] and r.last_deferred == len(fam["beyond"])
    # the second layer of a fusion: the uploaded region is reused, the index is not checked again, the answers are the same
    cached = r._on_device[0]
    di2, dw2 = r.relate(fam["queries"][::-1], device=0)
    assert r._on_device[0] is cached and cached["checked"]
    assert di2.tolist() == hi.tolist()[::-1] and dw2.tolist() == hw.tolist()[::-1]


def test_all_queries_in_one_launch():
    """Every query of every family against the first family's region in ONE launch (thousands of vertices of mixed sizes, several
    workgroups): still the host's flags, and only the rings beyond the vertex capacity are deferred."""
    r = Region(RC.FOREST)
    queries = [q for fam in FAMILIES if "UTM" not in fam["name"] for q in fam["queries"]]
    hi, hw = r.relate(queries)
    di, dw = r.relate(queries, device=0)
    assert di.tolist() == hi.tolist() and dw.tolist() == hw.tolist()
    assert r.last_deferred_queries.tolist() == [i for i, q in enumerate(queries) if len(q) > RC.QCAP]


def test_refused_rings_raise_before_any_launch(monkeypatch):
    lib = _lib.load()

    def launched(*a):
        raise AssertionError("td_region_relate_dev was called")

    r = Region(RC.FOREST)
    good = RC.sq(1, 1, 2, 2)
    r.relate([good], device=0)                       # the region is uploaded; from here on a launch would be the only GPU work
    monkeypatch.setattr(lib, "td_region_relate_dev", launched)
    for ring in (good[:4], good[[0, 1, 0]], np.array([[np.nan, 1], [2, 1], [2, 2], [np.nan, 1]])):       # not closed, three points, a NaN
        with pytest.raises(_lib.TdError, match="not a closed ring"):
            r.relate([good, ring], device=0)


def _raw_call(lib, r, index, queries, check_index=1):
    import torch

    edge_ring, bin_start, bin_edges, ymin, ymax, inv_h = index
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q_start = np.zeros(len(queries) + 1, np.int64)
    q_start[1:] = np.cumsum([len(q) for q in queries])
    q_xy = np.concatenate(queries)
    keep = [up(a) for a in (r.xy, r.ring_start, r.ring_poly, edge_ring, bin_start, bin_edges, q_xy, q_start)]
    flags = torch.zeros(len(queries), dtype=torch.uint8, device="cuda")
    status = torch.full((len(queries),), -7, dtype=torch.int32, device="cuda")
    st = lib.td_region_relate_dev(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), r.n_rings, len(r.xy), keep[3].data_ptr(),
                                  keep[4].data_ptr(), keep[5].data_ptr(), len(bin_start) - 1, len(bin_edges), ymin, ymax, inv_h,
                                  keep[6].data_ptr(), keep[7].data_ptr(), len(queries), len(q_xy), flags.data_ptr(), status.data_ptr(),
                                  check_index, _lib.stream_ptr())
    torch.cuda.synchronize()
    return st, flags.cpu().numpy(), status.cpu().numpy()


def test_an_index_that_points_past_the_edge_array_is_refused_not_read():
    lib = _lib.load()
    r = Region(RC.FOREST)
    queries = [c[1] for c in RC.KNOWN]
    index = vector.build_edge_index(r.xy, r.ring_start)
    st, flags, status = _raw_call(lib, r, index, queries)
    assert st == 0 and (status == 0).all() and (flags & 1).astype(bool).tolist() == [c[2] for c in RC.KNOWN]
    edge_ring, bin_start, bin_edges, *rest = index
    for what, bad_start, bad_edges, say in (
            ("an edge id past the vertices", bin_start, np.where(np.arange(len(bin_edges)) == 5, len(r.xy) + 1000, bin_edges).astype(np.int32), b"past the edge array"),
            ("the last vertex is no edge", bin_start, np.where(np.arange(len(bin_edges)) == 5, len(r.xy) - 1, bin_edges).astype(np.int32), b"past the edge array"),
            ("a negative edge id", bin_start, np.where(np.arange(len(bin_edges)) == 0, -3, bin_edges).astype(np.int32), b"past the edge array"),
            ("a bin that ends past the list", np.where(np.arange(len(bin_start)) == len(bin_start) - 1, len(bin_edges) + 64, bin_start).astype(np.int32),
             bin_edges, b"bin_start"),
            ("a ring's closing vertex as an edge", bin_start, np.where(np.arange(len(bin_edges)) == 0, 4, bin_edges).astype(np.int32), b"edge_ring")):
        st, flags, status = _raw_call(lib, r, (edge_ring, bad_start, bad_edges, *rest), queries)
        assert st == _lib.ERR_INVALID and say in lib.td_last_error(), what
        assert (status[1:] == -7).all() and not flags.any(), what           # the predicates were not launched


def test_argument_checks():
    lib = _lib.load()
    r = Region(RC.FOREST)
    edge_ring, bin_start, bin_edges, ymin, ymax, inv_h = vector.build_edge_index(r.xy, r.ring_start)
    ok = [1, 1, 1, r.n_rings, len(r.xy), 1, 1, 1, len(bin_start) - 1, len(bin_edges), ymin, ymax, inv_h, 1, 1, 1, 5, 1, 1, 0, None]
    # (pointer arguments are never followed: every call below is refused before anything is launched)
    for pos in (0, 1, 2, 5, 6, 7, 13, 14, 17, 18):
        a = list(ok)
        a[pos] = None
        assert lib.td_region_relate_dev(*a) == _lib.ERR_INVALID and b"null" in lib.td_last_error()
    for pos, value, say in ((3, 0, b"n_rings"), (4, 2 ** 31 - 1, b"n_vertices"), (8, 0, b"n_bins"), (9, 2 ** 31 - 1, b"n_bin_edges"), (15, -1, b"n_queries"),
                            (10, float("nan"), b"ymin"), (12, float("inf"), b"inv_h"), (11, ymin - 1, b"ymin <= ymax")):
        a = list(ok)
        a[pos] = value
        assert lib.td_region_relate_dev(*a) == _lib.ERR_INVALID and say in lib.td_last_error(), say
    a = list(ok)
    a[0], a[13] = 16, 24
    assert lib.td_region_relate_dev(*a) == _lib.ERR_INVALID and b"aligned" in lib.td_last_error()
    a = list(ok)
    a[0], a[13], a[15] = 16, 32, 0
    assert lib.td_region_relate_dev(*a) == 0                               # no queries: nothing is launched
