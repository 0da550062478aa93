"""The crafted outline configurations of tests/region_cases.py against the exact rational oracle AND the host td_region_relate
(no GPU), so that tests/test_region_relate_gpu.py compares the device kernel with answers known to be right — and the parts of the
device path that need no GPU: the binding, Region.relate's new argument, the config key, the edge index."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import region_cases as RC  # noqa: E402
from oracle import region_ref as O  # noqa: E402
from treedetection_amd import _lib, vector  # noqa: E402
from treedetection_amd.fusion import device_outlines_setting, exclude_outlines, fuse_predictions  # noqa: E402
from treedetection_amd.vector import Region  # noqa: E402

FAMILIES = RC.families()


def test_the_families_the_issue_lists_are_there():
    names = [f["name"] for f in FAMILIES]
    assert len(names) == len(set(names))
    assert sum(n.startswith("lattice") and "UTM" not in n for n in names) == 8 and sum(n.startswith("lattice") and "UTM" in n for n in names) == 8
    assert len(FAMILIES[0]["queries"]) == 17 and len(FAMILIES[1]["queries"]) == 17
    by = {f["name"]: f for f in FAMILIES}
    sizes = sorted({len(q) for q in by["query sizes"]["queries"]})
    assert sizes == [63, 64, 65, RC.QCAP - 1, RC.QCAP, RC.QCAP + 1]
    assert [len(q) > RC.QCAP for q in by["query sizes"]["queries"]] == [i in by["query sizes"]["beyond"] for i in range(len(by["query sizes"]["queries"]))]
    assert by["comb: meetings on one query edge"]["beyond"] == [3] and by["rings met by one query"]["beyond"] == [3]
    assert all(not f["beyond"] for f in FAMILIES if f["name"] not in ("query sizes", "comb: meetings on one query edge", "rings met by one query"))


@pytest.mark.parametrize("fam", FAMILIES, ids=[f["name"] for f in FAMILIES])
def test_family_against_oracle_and_host(fam):
    gi, gw = Region(fam["forest"]).relate(fam["queries"])
    got = list(zip(gi.tolist(), gw.tolist()))
    assert got == [O.relate(fam["forest"], q) for q in fam["queries"]]
    if fam["want"] is not None:
        assert got == fam["want"]
    if fam["mixed"]:
        assert 0 < sum(gi) < len(got) and 0 < sum(gw) < sum(gi)          # all three outcomes occur


def test_comb_and_rings_count_what_they_claim():
    """k meetings on one query edge / k rings met, counted with the oracle's own exact meeting routine."""
    by = {f["name"]: f for f in FAMILIES}
    fam = by["comb: meetings on one query edge"]
    edges = [(c, d) for poly in fam["forest"] for r in poly for c, d in zip(O._fr(r)[:-1], O._fr(r)[1:])]
    counts = []
    for q in fam["queries"]:
        a, b = O._fr(q)[0], O._fr(q)[1]
        counts.append(sum(len(O._meet_params(a, b, c, d)) for c, d in edges))
    assert counts == [3, RC.MCAP - 1, RC.MCAP, RC.MCAP + 1]
    fam = by["rings met by one query"]
    met = []
    for q in fam["queries"]:
        Q = O._fr(q)
        met.append(sum(any(O._meet_params(a, b, c, d) for a, b in zip(Q[:-1], Q[1:]) for r in poly for c, d in zip(O._fr(r)[:-1], O._fr(r)[1:]))
                       for poly in fam["forest"]))
    assert met == [2, RC.RCAP - 1, RC.RCAP, RC.RCAP + 1]


def test_dense_bins_hold_more_than_a_wave():
    fam = {f["name"]: f for f in FAMILIES}["dense bins"]
    r = Region(fam["forest"])
    _, bin_start, bin_edges, *_ = vector.build_edge_index(r.xy, r.ring_start)
    assert np.diff(bin_start).min() > 128


# ---- what fails without the feature ----------------------------------------------------------------------------------------------
def test_lib_binds_the_device_entry_and_the_capacities():
    assert "td_region_relate_dev" in _lib.SIGNATURES and len(_lib.SIGNATURES["td_region_relate_dev"][1]) == 21
    assert (_lib.RELATE_QUERY_CAP, _lib.RELATE_MEET_CAP, _lib.RELATE_RING_CAP) == (256, 254, 64)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "treedet.h")).read()
    for name, value in (("QUERY", 256), ("MEET", 254), ("RING", 64)):
        assert f"#define TD_RELATE_{name}_CAP {value} " in header
    assert "td_region_relate_dev(" in header


def test_relate_takes_device_none_and_returns_what_it_returned():
    r = Region(RC.FOREST)
    qs = [c[1] for c in RC.KNOWN]
    i0, w0 = r.relate(qs)
    i1, w1 = r.relate(qs, device=None)
    assert i1.dtype == bool and w1.dtype == bool and i1.tolist() == i0.tolist() == [c[2] for c in RC.KNOWN]
    assert w1.tolist() == w0.tolist() == [c[3] for c in RC.KNOWN]
    assert r.last_deferred == 0 and r._index is None and r._on_device == {}       # the host path builds and uploads nothing
    import inspect
    assert inspect.signature(fuse_predictions).parameters["device"].default is None
    assert "device_outlines" in (exclude_outlines.__doc__ or "")


def test_device_outlines_setting():
    assert device_outlines_setting(True) is True and device_outlines_setting("true") is True
    assert device_outlines_setting(False) is False and device_outlines_setting("false") is False and device_outlines_setting() is False
    assert device_outlines_setting(None) is False
    for bad in ("auto", 1.5, 1, 0, "yes"):
        with pytest.raises(ValueError, match="device_outlines must be true or false"):
            device_outlines_setting(bad)
    from treedetection_amd.fusion import outline_device
    assert outline_device({"device": "0"}) is None and outline_device({"device_outlines": False, "device": "cpu"}) is None
    with pytest.raises(ValueError, match="device_outlines"):
        outline_device({"device_outlines": True, "device": "cpu"})


# ---- the edge index the device path uploads ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["known answers", "lattice 3 at UTM", "dense bins", "comb: meetings on one query edge"])
def test_edge_index_lists_every_edge_in_every_bin_it_touches(name):
    fam = {f["name"]: f for f in FAMILIES}[name]
    r = Region(fam["forest"])
    edge_ring, bin_start, bin_edges, ymin, ymax, inv_h = vector.build_edge_index(r.xy, r.ring_start)
    nb = len(bin_start) - 1
    n_edges = len(r.xy) - r.n_rings
    assert nb == min(8192, max(1, n_edges // 4)) and bin_start[0] == 0 and bin_start[-1] == len(bin_edges)
    assert edge_ring.dtype == np.int32 and bin_start.dtype == np.int32 and bin_edges.dtype == np.int32
    assert (ymin, ymax) == (r.xy[:, 1].min(), r.xy[:, 1].max())

    def bin_of(y):                                   # csrc/geom_predicates.h: relate_bin_of
        f = (y - ymin) * inv_h
        return 0 if not f > 0 else (nb - 1 if f >= nb else int(f))

    want = [[] for _ in range(nb)]
    for ring in range(r.n_rings):
        for i in range(r.ring_start[ring], r.ring_start[ring + 1] - 1):
            assert edge_ring[i] == ring
            y0, y1 = sorted((r.xy[i, 1], r.xy[i + 1, 1]))
            for b in range(bin_of(y0), bin_of(y1) + 1):
                want[b].append(i)
    assert [bin_edges[bin_start[b]:bin_start[b + 1]].tolist() for b in range(nb)] == want


def test_device_path_declines_before_it_needs_a_gpu(capsys):
    r = Region(RC.FOREST)
    bad = RC.sq(1, 1, 2, 2)
    bad[2, 0] = np.nan
    i, w = r.relate([RC.sq(1, 1, 2, 2), bad], device=0)                   # a NaN inside a closed ring: the host function serves
    assert "Region.relate: a coordinate is not finite: using the host function" in capsys.readouterr().out
    assert i.tolist() == r.relate([RC.sq(1, 1, 2, 2), bad])[0].tolist()
    i, w = Region([]).relate([RC.sq(1, 1, 2, 2)], device=0)
    assert not i.any() and not w.any() and "the region is empty" in capsys.readouterr().out
    for ring in (RC.sq(1, 1, 2, 2)[:4], RC.sq(1, 1, 2, 2)[[0, 1, 0]], np.array([[np.nan, 1], [2, 1], [2, 2], [np.nan, 1]])):
        with pytest.raises(_lib.TdError, match="not a closed ring"):       # what the host call raises, device or not
            r.relate([RC.sq(1, 1, 2, 2), ring], device=0)
        with pytest.raises(_lib.TdError, match="not a closed ring"):
            r.relate([RC.sq(1, 1, 2, 2), ring])
