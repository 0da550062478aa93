"""``crown_statistics``: process_layer with the statistics over the bounding circles (absent key or "circle": the reference's, as
before) and over the crown outlines ("polygon": td_crown_zonal_dev) on a small layer built to tell them apart — a short, elongated
crown beside one tall pixel that lies inside the crown's circle but outside its ring, and an elongated crown on low-NDVI ground
whose circle takes in the ground. The circle results are compared with a recording of crown_stats, not with stored numbers; the
polygon results with the exact pixel sets of zonal_cases.py."""
import numpy as np
import pytest

from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import write_geotiff

import zonal_cases as Z

pytestmark = pytest.mark.gpu

SIDE = 300                                                  # RGBI pixels of 0.2 m; the nDSM and (ndvi_scaling_factor 0.2) the NDVI raster have 1 m pixels
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318120.0)
HEIGHT_THR, NDVI_MEAN_THR = 3.0, 0.35
TALL = 25.0


def _rect(x0, y0, x1, y1):
    """A closed ring in map coordinates from nDSM pixel units (x to the east, y to the SOUTH of the raster's corner)."""
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return np.array([(NT[2] + x, NT[5] - y) for x, y in pts])


def _scene():
    """West half: vegetated ground (high NDVI) with crown A, 14 m x 3 m and 6 m high, and a 25 m pixel 4 m north of its middle.
    East half: bare ground (low NDVI) with crown B, 14 m x 4 m and 8 m high, of high NDVI itself."""
    n = SIDE // 5
    rgbi = np.zeros((4, SIDE, SIDE), np.uint8)
    rgbi[0], rgbi[3] = 40, 220                               # vegetation: NDVI about 0.69
    rgbi[0, :, SIDE // 2:], rgbi[3, :, SIDE // 2:] = 200, 20          # bare: about -0.82
    rgbi[1], rgbi[2] = 90, 70
    rng = np.random.default_rng(5)
    ndsm = rng.uniform(0.0, 0.5, (n, n)).astype(np.float32)
    a = (8.3, 28.4, 22.3, 31.4)                              # crown A: x 8.3 .. 22.3, y 28.4 .. 31.4 (metres from the corner)
    b = (37.3, 20.2, 51.3, 24.2)                             # crown B
    ndsm[29:31, 9:22] = rng.uniform(5.0, 6.0, (2, 13)).astype(np.float32)
    ndsm[25, 15] = TALL                                      # centre (15.5, 25.5): 4.4 m north of A's middle, outside its ring
    ndsm[21:24, 38:51] = rng.uniform(7.0, 8.0, (3, 13)).astype(np.float32)
    rgbi[0, int(b[1] * 5):int(b[3] * 5), int(b[0] * 5):int(b[2] * 5)] = 40
    rgbi[3, int(b[1] * 5):int(b[3] * 5), int(b[0] * 5):int(b[2] * 5)] = 220
    return rgbi, ndsm, [_rect(*a), _rect(*b)], [0.9, 0.8]


def _config(**extra):
    cfg = {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": HEIGHT_THR,
           "ndvi_mean_threshold": NDVI_MEAN_THR, "ndvi_var_threshold": 10.0, "use_overlap": False, "tile_width": 50, "tile_height": 50, "buffer": 10,
           "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": 0.2, "height_scaling_factor": 1.0}
    cfg.update(extra)
    return cfg


@pytest.fixture
def layer(tmp_path):
    rgbi, ndsm, rings, scores = _scene()
    rpath, hpath = str(tmp_path / "rgbi.tif"), str(tmp_path / "ndsm.tif")
    write_geotiff(rpath, rgbi, T, 25832, compression="deflate", tile=(128, 128))
    write_geotiff(hpath, ndsm[None], NT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    return rings, scores, hpath, rpath, ndsm


@pytest.fixture
def calls(monkeypatch):
    """Records what crown_stats and crown_zonal_stats return while process_layer runs."""
    seen = {"circle": [], "polygon": []}
    circle, polygon = P.crown_stats, P.crown_zonal_stats

    def rec_circle(*args, **kw):
        out = circle(*args, **kw)
        seen["circle"].append((args[4], out))                # (mode, statistics)
        return out

    def rec_polygon(*args, **kw):
        out = polygon(*args, **kw)
        seen["polygon"].append(out)
        return out
    monkeypatch.setattr(P, "crown_stats", rec_circle)
    monkeypatch.setattr(P, "crown_zonal_stats", rec_polygon)
    return seen


def _same_features(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


def test_circle_and_absent_key_keep_the_circle_statistics(layer, calls):
    rings, scores, hpath, rpath, ndsm = layer
    absent = P.process_layer(rings, scores, _config(), hpath, rpath)
    heights = next(out for mode, out in calls["circle"] if mode == 0)
    ndvi = next(out for mode, out in calls["circle"] if mode == 1)
    print(f"circle: heights {heights[:, 0].tolist()}, NDVI means {ndvi[:, 2].tolist()}")
    assert len(calls["circle"]) == 2 and not calls["polygon"]
    # crown A comes out with the tall pixel's value, which its ring does not hold; crown B's circle takes in the bare ground
    assert heights[0, 0] == np.float32(TALL) and ndvi[0, 2] > NDVI_MEAN_THR + 0.05 and ndvi[1, 2] < NDVI_MEAN_THR - 0.05
    assert [f["properties"]["poly_id"] for f in absent] == ["0"]
    assert absent[0]["properties"]["TreeHeight"] == float(heights[0, 0]) == TALL
    del calls["circle"][:]
    circle = P.process_layer(rings, scores, _config(crown_statistics="circle"), hpath, rpath)
    assert len(calls["circle"]) == 2 and not calls["polygon"]
    _same_features(absent, circle)
    _same_features(absent, P.process_layer(rings, scores, _config(crown_statistics=None), hpath, rpath))


def test_polygon_measures_the_crown_itself(layer, calls):
    rings, scores, hpath, rpath, ndsm = layer
    feats = P.process_layer(rings, scores, _config(crown_statistics="polygon"), hpath, rpath)
    assert len(calls["polygon"]) == 2 and not calls["circle"]
    (h_stats, h_count, h_pos, h_status), (n_stats, n_count, _, n_status) = calls["polygon"]
    print(f"polygon: heights {h_stats[:, 1].tolist()}, NDVI means {n_stats[:, 2].tolist()}, counts {h_count.tolist()} / {n_count.tolist()}")
    assert (h_status == 0).all() and (n_status == 0).all()
    # the crown's own maximum: over exactly the nDSM pixels whose centres the exact oracle puts inside the ring
    X, Y = Z.centres(NT, *ndsm.shape)
    for k, ring in enumerate(rings):
        pix = Z.pixels_inside(ring[:-1], X, Y)
        assert len(pix) == h_count[k] > 0
        assert (25, 15) not in pix
        own = max(ndsm[r, c] for r, c in pix)
        assert h_stats[k, 1] == own and ndsm[tuple(h_pos[k])] == own
    assert h_stats[0, 1] < 6.0 + 1e-6 and h_stats[1, 1] < 8.0 + 1e-6
    assert (n_stats[:, 2] > NDVI_MEAN_THR + 0.05).all()      # both crowns are vegetation, measured on themselves
    assert [f["properties"]["poly_id"] for f in feats] == ["0", "1"]          # crown B is kept only under polygon
    assert [f["properties"]["TreeHeight"] for f in feats] == [float(h_stats[0, 1]), float(h_stats[1, 1])]


def test_an_invalid_value_raises(layer):
    rings, scores, hpath, rpath, _ = layer
    for bad in ("polygons", True, 1):
        with pytest.raises(ValueError, match="crown_statistics must be 'circle' or 'polygon'"):
            P.process_layer(rings, scores, _config(crown_statistics=bad), hpath, rpath)
