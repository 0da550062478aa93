"""``crown_rasters``: the label raster beside a processed layer. A small scene — a 300 x 300 RGBI image of 0.2 m pixels, a 60 x 60
nDSM of 1 m pixels, five crowns, two of them overlapping with different scores and another overlapping pair with EQUAL scores.
Absent or false: no raster, the same layer. "height" / "image": the same layer, and a uint32 raster on that file's grid whose pixels
equal the label_cases expectation built from the rings and scores READ BACK from the processed layer (the exact oracle's pixel
sets; the higher score on top, among equal scores the lower row). postprocess_files copies it next to the layer.

Layers are compared byte for byte with one field made equal first: GeoPackage's ``gpkg_contents.last_change``, the wall-clock
time of the write to the millisecond, which differs between any two writes of the same layer."""
import os
import shutil
import sqlite3

import numpy as np
import pytest

import treedetection_amd as T
from treedetection_amd import gpkg
from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff

import label_cases as L

pytestmark = pytest.mark.gpu

SIDE = 300
IT = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)             # the image: 300 x 300 pixels of 0.2 m
HT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318120.0)             # the nDSM: 60 x 60 pixels of 1 m
NAME = "3241"


def _ring(points):
    """A closed ring in map coordinates from metres east and SOUTH of the rasters' corner."""
    pts = list(points) + [points[0]]
    return np.array([(HT[2] + x, HT[5] - y) for x, y in pts])


def _hexagon(cx, cy, r):
    return [(cx + r * np.cos(a), cy + r * np.sin(a)) for a in np.deg2rad([10, 70, 130, 190, 250, 310])]


CROWNS = [(_hexagon(14.0, 14.0, 7.0), 0.9),                                         # A
          (_hexagon(22.3, 17.1, 6.0), 0.6),                                         # B: reaches into A, the lower score
          ([(34.3, 30.2), (46.7, 31.1), (45.9, 40.6), (35.2, 39.8)], 0.7),          # C
          ([(41.2, 35.3), (53.6, 36.4), (52.8, 47.9), (42.1, 46.6)], 0.7),          # D: reaches into C, the same score
          ([(10.2, 38.4), (23.7, 41.3), (14.6, 53.2)], 0.5)]                        # E: alone


def _scene(root):
    os.makedirs(root / "img")
    os.makedirs(root / "ndsm")
    pred = root / "out" / "geojson_predictions"
    os.makedirs(pred)
    rgbi = np.zeros((4, SIDE, SIDE), np.uint8)
    rgbi[0], rgbi[1], rgbi[2], rgbi[3] = 40, 90, 70, 220     # vegetation everywhere: NDVI about 0.69
    rng = np.random.default_rng(5)
    ndsm = rng.uniform(5.0, 9.0, (SIDE // 5, SIDE // 5)).astype(np.float32)         # and tall everywhere: every crown passes
    write_geotiff(str(root / "img" / f"{NAME}.tif"), rgbi, IT, 25832, compression="deflate", tile=(128, 128))
    write_geotiff(str(root / "ndsm" / f"{NAME}.tif"), ndsm[None], HT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    gpkg.write_polygons(str(pred / f"{NAME}.gpkg"), [_ring(p) for p, _ in CROWNS], {"Confidence_score": [s for _, s in CROWNS]}, 25832)
    return pred


class _Log:
    def __getattr__(self, name):
        return lambda m: None


def _config(root, **extra):
    cfg = {"logger": _Log(), "output_directory": str(root / "out"), "height_data_path": str(root / "ndsm"), "image_directory": str(root / "img"),
           "confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 3,
           "ndvi_mean_threshold": 0.35, "ndvi_var_threshold": 10.0, "use_overlap": False, "tile_width": 50, "tile_height": 50, "buffer": 10,
           "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "device": "0", "parallel": False, "exclude_files": [],
           "confidence_threshold_stitching": 0.3, "timestamped_output_directory": False, "ndvi_scaling_factor": 0.2, "height_scaling_factor": 1.0}
    cfg.update(extra)
    return cfg


def _layer_bytes(path):
    """The file's bytes with gpkg_contents.last_change (the time of the write) made the same in every file."""
    con = sqlite3.connect(path)
    stamps = [r[0] for r in con.execute("SELECT last_change FROM gpkg_contents")]
    con.close()
    raw = open(path, "rb").read()
    assert len(stamps) == 1 and len(stamps[0]) == 24 and raw.count(stamps[0].encode()) == 1
    return raw.replace(stamps[0].encode(), b"T" * 24)


def _single(root, tag, **extra):
    """process_single_file into a folder of its own → (path of the processed layer, folder)."""
    out = root / tag
    os.makedirs(out)
    layer = str(out / f"processed_{NAME}.gpkg")
    res = P.process_single_file(str(root / "out" / "geojson_predictions" / f"{NAME}.gpkg"), layer, str(root / "ndsm" / f"{NAME}.tif"),
                                str(root / "img" / f"{NAME}.tif"), device_id="0", config=_config(root, **extra))
    assert res is not None
    return layer, out


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("labels")
    _scene(root)
    off, off_dir = _single(root, "false", crown_rasters=False)
    return root, off, off_dir


def test_absent_and_false_write_no_raster_and_the_same_layer(scene):
    root, off, off_dir = scene
    absent, absent_dir = _single(root, "absent")
    none, none_dir = _single(root, "none", crown_rasters=None)
    for d in (off_dir, absent_dir, none_dir):
        assert sorted(os.listdir(d)) == [f"processed_{NAME}.gpkg"]
    assert _layer_bytes(absent) == _layer_bytes(off) == _layer_bytes(none)
    rings, cols, _ = gpkg.read_polygons(off)
    assert len(rings) == len(CROWNS) and cols["Confidence_score"] == [s for _, s in CROWNS]          # the scene keeps all five crowns


@pytest.mark.parametrize("mode", ["height", "image"])
def test_the_raster_holds_the_layers_crowns(scene, mode):
    root, off, _ = scene
    layer, out = _single(root, mode, crown_rasters=mode)
    assert sorted(os.listdir(out)) == [f"processed_{NAME}.gpkg", f"processed_{NAME}_crowns.tif"]
    assert _layer_bytes(layer) == _layer_bytes(off)
    src = GeoTiff(str(root / ("ndsm" if mode == "height" else "img") / f"{NAME}.tif"))
    g = GeoTiff(str(out / f"processed_{NAME}_crowns.tif"))
    assert (g.height, g.width, g.count) == (src.height, src.width, 1) == ((60, 60, 1) if mode == "height" else (300, 300, 1))
    assert g.transform == src.transform == (HT if mode == "height" else IT) and g.epsg == src.epsg == 25832
    assert g.dtype == np.uint32 and g.nodata == 0.0 and g.compression == 5           # LZW
    labels = g.read()[0]
    assert not g._strips and (g._bh, g._bw) == (256, 256)                             # tiled
    g.close()
    src.close()
    rings, cols, _ = gpkg.read_polygons(layer)
    want = L.expected_from_layer(labels.shape, g.transform, rings, cols["Confidence_score"])
    counts = np.bincount(labels.reshape(-1), minlength=len(rings) + 1)
    print(f"{mode}: pixels per label {counts.tolist()}")
    assert np.array_equal(labels, want), f"{int((labels != want).sum())} pixels differ"
    assert counts.size == len(rings) + 1 and (counts > 0).all()
    # the overlaps went to the right crown: A over B, and of the equal pair the earlier row
    for top, under in ((0, 1), (2, 3)):
        alone = L.expected_from_layer(labels.shape, g.transform, [rings[under]], [1.0])
        shared = (alone == 1) & (want == top + 1)
        assert shared.sum() > 0 and (labels[shared] == top + 1).all()


def test_postprocess_files_copies_the_raster_next_to_the_layer(tmp_path):
    pred = _scene(tmp_path)
    T.postprocess_files(_config(tmp_path, crown_rasters="height", timestamped_output_directory=True))
    out = tmp_path / "out"
    assert os.path.exists(pred / f"processed_{NAME}_crowns.tif") and os.path.exists(out / f"{NAME}.gpkg")
    a, b = open(pred / f"processed_{NAME}_crowns.tif", "rb").read(), open(out / f"{NAME}_crowns.tif", "rb").read()
    assert a == b and len(a) > 0
    stamped = [d for d in os.listdir(out) if os.path.isdir(out / d) and d not in ("geojson_predictions", "logs")]
    assert len(stamped) == 1 and sorted(os.listdir(out / stamped[0])) == [f"{NAME}.gpkg", f"{NAME}_crowns.tif"]
    g = GeoTiff(str(out / f"{NAME}_crowns.tif"))
    labels = g.read()[0]
    g.close()
    rings, cols, _ = gpkg.read_polygons(str(out / f"{NAME}.gpkg"))
    assert np.array_equal(labels, L.expected_from_layer((60, 60), HT, rings, cols["Confidence_score"]))
    # with the key off nothing of the kind appears
    shutil.rmtree(out)
    shutil.rmtree(tmp_path / "img")
    shutil.rmtree(tmp_path / "ndsm")
    _scene(tmp_path)
    T.postprocess_files(_config(tmp_path))
    assert os.path.exists(out / f"{NAME}.gpkg") and not [n for n in os.listdir(out) + os.listdir(pred) if n.endswith(".tif")]


def test_a_failure_to_draw_is_printed_and_keeps_the_layer(scene, monkeypatch, capsys):
    root, off, _ = scene

    def broken(*args, **kw):
        raise RuntimeError("no raster today")
    monkeypatch.setattr(P, "write_crown_raster", broken)
    layer, out = _single(root, "broken", crown_rasters="image")
    printed = capsys.readouterr().out
    assert "Error writing the crown raster" in printed and "no raster today" in printed
    assert sorted(os.listdir(out)) == [f"processed_{NAME}.gpkg"] and _layer_bytes(layer) == _layer_bytes(off)


def test_a_bad_value_is_refused(scene):
    root, _, _ = scene
    for k, bad in enumerate(("both", True, 1)):
        with pytest.raises(ValueError, match="crown_rasters must be false, 'height' or 'image'"):
            _single(root, f"bad{k}", crown_rasters=bad)
        assert not os.listdir(root / f"bad{k}")
