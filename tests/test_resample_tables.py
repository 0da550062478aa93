"""The tap tables td_resample_gdal_dev is fed (postprocessing.tap_tables): _decimation_weights entry for entry, and the host-side
validation that keeps a table reaching outside the source away from the kernels. No GPU."""
import numpy as np
import pytest

from treedetection_amd import postprocessing as P

AXES = [(317, 63), (203, 40), (203, 101), (64, 23), (97, 164), (131, 222), (7, 1), (5, 1), (20011, 4002), (3, 1), (256, 256), (1, 1), (2, 5)]


@pytest.mark.parametrize("n_src,n_dst", AXES)
def test_flattened_tables_reproduce_the_decimation_weights(n_src, n_dst):
    start, count, offset, weights = P.tap_tables(n_src, n_dst)
    rows = P._decimation_weights(n_src, n_dst)
    assert start.dtype == count.dtype == offset.dtype == np.int32 and weights.dtype == np.float32
    assert start.shape == count.shape == offset.shape == (n_dst,) == (len(rows),)
    assert weights.size == int(count.sum()) and int(offset[0]) == 0
    for j, (idx, wgt) in enumerate(rows):
        assert np.array_equal(np.arange(start[j], start[j] + count[j]), idx), j
        assert np.array_equal(weights[offset[j]:offset[j] + count[j]].view(np.uint32), wgt.astype(np.float32).view(np.uint32)), j
    P.check_tap_tables((start, count, offset, weights), n_src, n_dst)


def test_identity_taps_are_one_and_zero():
    start, count, offset, weights = P.tap_tables(256, 256)
    assert np.array_equal(start, np.arange(256)) and (count[:-1] == 2).all() and count[-1] == 1
    assert (weights[offset] == 1.0).all() and (weights[offset[:-1] + 1] == 0.0).all()


def _broken(n_src, n_dst, **change):
    t = dict(zip(("start", "count", "offset", "weights"), (a.copy() for a in P.tap_tables(n_src, n_dst))))
    for name, (j, v) in change.items():
        t[name][j] = v
    return t["start"], t["count"], t["offset"], t["weights"]


@pytest.mark.parametrize("change,what", [
    ({"start": (0, -1)}, "outside the 317 source"),
    ({"start": (62, 312)}, "outside the 317 source"),                 # the last output's ten taps would end at 322
    ({"count": (5, 0)}, "outside the 317 source"),
    ({"count": (62, 11)}, "outside the 317 source"),
    ({"start": (3, 2 ** 31 - 1)}, "outside the 317 source"),          # no wrap-around in start + count
    ({"offset": (62, 10 ** 6)}, "outside its"),
    ({"offset": (0, -1)}, "outside its"),
])
def test_a_table_reaching_outside_is_refused_on_the_host(change, what):
    with pytest.raises(ValueError, match=what):
        P.check_tap_tables(_broken(317, 63, **change), 317, 63, "x")


def test_wrong_types_and_lengths_are_refused():
    start, count, offset, weights = P.tap_tables(64, 23)
    for bad in ((start.astype(np.int64), count, offset, weights), (start[:-1], count, offset, weights), (start, count, offset, weights.astype(np.float64)),
                (start, count, list(offset), weights), (start, count, offset, weights[:0])):
        with pytest.raises(ValueError, match="tap table"):
            P.check_tap_tables(bad, 64, 23)


def test_the_wrapper_validates_before_it_touches_a_device(monkeypatch):
    """resample_on_device validates the tables on the host, before it asks for a device: a host tensor with a crafted table is
    refused for the table, one with good tables for being a host tensor — and the library is never loaded."""
    import torch
    from treedetection_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    raster = torch.zeros((317, 203, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="x tap table reaches outside the 203 source"):
        P.resample_on_device(raster, 63, 40, [0, 3], "ndvi", tables=(_broken(203, 40, start=(39, 200)), P.tap_tables(317, 63)))
    with pytest.raises(ValueError, match="y tap table reaches outside the 317 source"):
        P.resample_on_device(raster, 63, 40, [0, 3], "ndvi", tables=(P.tap_tables(203, 40), _broken(317, 63, count=(62, 11))))
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        P.resample_on_device(raster, 63, 40, [0, 3], "ndvi")
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        P.resample_on_device(raster.double(), 63, 40, [0, 3], "ndvi")
    with pytest.raises(ValueError, match="cannot resample"):
        P.resample_on_device(raster, 0, 40, [0, 3], "ndvi")
    with pytest.raises(ValueError, match="mode"):
        P.resample_on_device(raster, 63, 40, [0, 3], "u16")
