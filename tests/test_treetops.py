"""td_treetops, the host twin of the treetop kernel, and the Python layer above it, without a GPU: marks and smoothed raster against
the numpy oracle of tests/treetop_cases.py bit for bit on every case, against live scipy where it is installed and against recorded
scipy results where it is not, error returns, the point blobs and the point layer of the GeoPackage writer."""
import ctypes as C
import os
import sqlite3

import numpy as np
import pytest

import treetop_cases as tc
from treedetection_amd import _lib, gpkg, treetops as tt


def host(raster, w, k, floor, counts=False):
    m, s, c = tt._run(np.ascontiguousarray(raster, np.float32), w, k, floor, None, True, counts, "test")
    return (m, s, c) if counts else (m, s)


def check_against_oracle(name, raster, w, k, floor):
    marks, smoothed, counts = host(raster, w, k, floor, counts=True)
    want_marks, want_smoothed = tc.oracle(raster, w, k, floor)
    assert tc.same_floats(smoothed, want_smoothed), name
    assert marks.dtype == np.uint8 and (marks == want_marks).all(), (name, np.argwhere(marks != want_marks)[:5])
    assert (counts == want_marks.sum(axis=1)).all(), name
    return marks


@pytest.mark.parametrize("shape", tc.SHAPES, ids=[f"{r}x{c}" for r, c in tc.SHAPES])
def test_host_twin_equals_the_oracle_on_random_and_plateau_rasters(shape):
    found = 0
    for name, raster, w, k, floor in tc.random_cases(shape):
        found += int(check_against_oracle(name, raster, w, k, floor).sum())
    assert found > 0 or shape == (1, 1)


def test_host_twin_equals_the_oracle_on_crafted_rasters():
    for name, raster, w, k, floor, expected in tc.crafted_cases():
        marks = check_against_oracle(name, raster, w, k, floor)
        if expected is not None:
            assert sorted(map(tuple, np.argwhere(marks))) == sorted(expected), name


def test_weights_are_scipys_table():
    for sigma in (0.0, 0.3, 0.5, 1.0, 2.0, 2.7):
        assert (tt.gaussian_weights(sigma) == tc.weights(sigma)).all()
    ndimage = pytest.importorskip("scipy.ndimage")
    for sigma in (0.5, 1.0, 2.0, 2.7):
        r = int(4.0 * sigma + 0.5)
        impulse = np.zeros(4 * r + 1)
        impulse[2 * r] = 1.0                                           # scipy's own table, read back off a unit impulse: 1.0 * w is exact
        assert (tt.gaussian_weights(sigma) == ndimage.gaussian_filter1d(impulse, sigma, mode="constant")[r:3 * r + 1]).all()
    with pytest.raises(ValueError):
        tt.gaussian_weights(-1.0)
    with pytest.raises(ValueError):
        tt.gaussian_weights(float("nan"))


def test_host_twin_equals_live_scipy_on_nan_free_rasters():
    nd = pytest.importorskip("scipy.ndimage")
    for shape in tc.SHAPES:
        for sigma in (0.5, 1.0, 2.0):
            for k in (3, 7):
                raster = tc.canopy(shape, 31 * tc.SHAPES.index(shape) + k, plateaus=shape[0] > 16)
                s = nd.gaussian_filter(raster, sigma=sigma)
                assert tc.same_floats(tt.smooth_height(raster, sigma, device=None), s), (shape, sigma)
                rows, cols, height, xy = tt.find_treetops(raster, None, sigma, k, tc.FLOOR, device=None)
                want = np.argwhere((s == nd.maximum_filter(s, size=k)) & (s > np.float32(tc.FLOOR)))
                assert xy is None and (np.stack([rows, cols], axis=1) == want).all(), (shape, sigma, k)
                assert tc.same_floats(height, s[want[:, 0], want[:, 1]])


def test_host_twin_equals_the_recorded_scipy_results():
    cases = tc.golden_cases()
    assert len(cases) >= 8
    total = 0
    for name, raster, sigma, k, floor, smoothed, tops in cases:
        assert tc.same_floats(tt.smooth_height(raster, sigma, device=None), smoothed), name
        rows, cols, height, _ = tt.find_treetops(raster, None, sigma, k, floor, device=None)
        assert (np.stack([rows, cols], axis=1).reshape(-1, 2) == tops.reshape(-1, 2)).all(), name
        assert tc.same_floats(height, smoothed[tops[:, 0], tops[:, 1]]), name
        total += len(rows)
    assert total > 100


def test_find_treetops_places_pixel_centres():
    raster = tc.spike((6, 8), [(1, 2), (4, 6)])
    t = (0.5, 0.0, 100.0, 0.0, -0.5, 200.0)
    rows, cols, height, xy = tt.find_treetops(raster, t, sigma=0.0, window=3, min_height=3.0, device=None)
    assert rows.tolist() == [1, 4] and cols.tolist() == [2, 6] and height.tolist() == [10.0, 10.0]
    assert xy.tolist() == [[101.25, 199.25], [103.25, 197.75]]
    marks = tt.treetop_marks(raster, sigma=0.0, window=3, device=None)
    assert isinstance(marks, np.ndarray) and marks.dtype == np.uint8 and marks.sum() == 2


def test_malformed_calls_are_refused_with_a_message():
    lib = _lib.load()
    raster = np.ones((4, 5), np.float32)
    marks = np.zeros((4, 5), np.uint8)
    w = tt.gaussian_weights(0.5)

    def call(r=raster.ctypes.data, rows=4, cols=5, wt=w, radius=2, window=7, floor=3.0, m=marks.ctypes.data):
        wt = None if wt is None else np.ascontiguousarray(wt, np.float64)
        return lib.td_treetops(r, rows, cols, None if wt is None else wt.ctypes.data, radius, window, floor, m, None, None)

    assert call() == 0
    bad = dict(r=dict(r=None), w=dict(wt=None), m=dict(m=None), rows=dict(rows=0), cols=dict(cols=-1), pixels=dict(rows=1 << 16, cols=1 << 15),
               even=dict(window=6), zero=dict(window=0), negative=dict(window=-3), radius=dict(radius=-1), floor=dict(floor=float("nan")),
               nan_weight=dict(wt=[0.1, np.nan, 0.8, np.nan, 0.1]), inf_weight=dict(wt=[np.inf, 0.1, 0.8, 0.1, np.inf]),
               asymmetric=dict(wt=[0.1, 0.2, 0.4, 0.2, 0.15]))
    for name, kw in bad.items():
        marks[:] = 7
        assert call(**kw) == _lib.ERR_INVALID, name
        assert lib.td_last_error().startswith(b"td_treetops:"), name
        assert (marks == 7).all(), name                               # before anything runs
    with pytest.raises(_lib.TdError):
        tt.treetop_marks(raster, min_height=float("nan"), device=None)
    with pytest.raises(_lib.TdError):
        tt.treetop_marks(raster, window=4, device=None)
    with pytest.raises(ValueError):
        tt.treetop_marks(np.ones(5, np.float32), device=None)


def test_point_blob_round_trip():
    for x, y, srs in ((0.0, 0.0, 4326), (389012.125, 5819999.875, 25833), (-1e-300, 1e300, -1)):
        blob = gpkg.point_blob(x, y, srs)
        assert len(blob) == 8 + 21 and gpkg.parse_point_blob(blob) == (srs, (x, y))
    with pytest.raises(ValueError):
        gpkg.parse_point_blob(gpkg.polygon_blob(np.array([[0, 0], [1, 0], [1, 1], [0, 0]], float), 4326))
    with pytest.raises(ValueError):
        gpkg.parse_polygon_blob(gpkg.point_blob(1.0, 2.0, 4326))


def _dump(path):
    con = sqlite3.connect(path)
    try:
        return [row for row in con.execute("SELECT type, name, sql FROM sqlite_master ORDER BY name")] + \
               [row for t in ("gpkg_contents", "gpkg_geometry_columns", "gpkg_spatial_ref_sys")
                for row in con.execute(f"SELECT * FROM {t}") if t != "gpkg_contents"] + \
               [row[:3] + row[5:] for row in con.execute("SELECT * FROM gpkg_contents")]     # (without last_change)
    finally:
        con.close()


def test_the_polygon_writer_is_unchanged_by_the_new_argument(tmp_path):
    ring = np.array([[1.0, 2.0], [4.0, 2.0], [4.0, 6.0], [1.0, 2.0]])
    cols = {"Confidence_score": [0.5], "poly_id": ["0"], "n": [3]}
    a, b = str(tmp_path / "a" / "layer.gpkg"), str(tmp_path / "b" / "layer.gpkg")
    os.makedirs(os.path.dirname(a)), os.makedirs(os.path.dirname(b))
    gpkg.write_blobs(a, [gpkg.polygon_blob(ring, 25833)], cols, 25833, (1.0, 2.0, 4.0, 6.0))
    gpkg.write_blobs(b, [gpkg.polygon_blob(ring, 25833)], cols, 25833, (1.0, 2.0, 4.0, 6.0), geometry_type="POLYGON")
    assert _dump(a) == _dump(b)
    sql = [row[2] for row in _dump(a) if row[1] == "layer"][0]
    assert "geom POLYGON" in sql
    con = sqlite3.connect(a)
    assert con.execute("SELECT geometry_type_name FROM gpkg_geometry_columns").fetchone() == ("POLYGON",)
    assert con.execute('SELECT geom, "Confidence_score", poly_id, n FROM layer').fetchall() == [(gpkg.polygon_blob(ring, 25833), 0.5, "0", 3)]
    con.close()
    rings, got, srs = gpkg.read_polygons(a)
    assert (rings[0] == ring).all() and got == cols and srs == 25833
    with pytest.raises(ValueError):
        gpkg.write_blobs(a, [], {}, 25833, None, geometry_type="LINESTRING")


def test_treetop_layer_is_a_point_layer(tmp_path):
    path = str(tmp_path / "tops.gpkg")
    tops = {"rows": np.array([1, 4]), "cols": np.array([2, 6]), "height": np.array([10.0, 12.5], np.float32),
            "xy": np.array([[101.25, 199.25], [103.25, 197.75]]), "crown": np.array([2, 0])}
    tt.write_treetops_layer(path, tops, 25833)
    con = sqlite3.connect(path)
    assert con.execute("SELECT geometry_type_name, srs_id FROM gpkg_geometry_columns").fetchone() == ("POINT", 25833)
    rows = con.execute('SELECT geom, "Height", "Row", "Col", "Crown" FROM tops ORDER BY fid').fetchall()
    con.close()
    assert [gpkg.parse_point_blob(r[0]) for r in rows] == [(25833, (101.25, 199.25)), (25833, (103.25, 197.75))]
    assert [r[1:] for r in rows] == [(10.0, 1, 2, 2), (12.5, 4, 6, 0)]
    layer = gpkg.read_layer(path)
    assert len(layer) == 2 and layer.columns["Crown"] == [2, 0]
    tt.write_treetops_layer(path, {"rows": [], "cols": [], "height": [], "xy": np.zeros((0, 2))}, None)       # an empty layer is a layer
    assert len(gpkg.read_layer(path)) == 0
