"""``crown_treetops``: treetops counted per crown and written beside the processed layer. The scene of tests/treetop_cases.py — a
60 x 60 nDSM of 1 m pixels, flat at 2.5 m with six spikes, five crowns that hold 2, 1, 0, 1 and 2 of them, one spike under two
overlapping crowns and one under none. Absent or false: the same layer byte for byte and no other file. True: the same features
with an integer column ``Treetops`` as constructed, and a point layer whose rows, columns, heights and crowns are as constructed
and equal the host functions' (``device=None``); the same with the height raster decoded in HBM and with a scaled height raster;
a failure is printed and keeps the layer; postprocess_files copies the point layer next to the layer.

Layers are compared byte for byte with one field made equal first: GeoPackage's ``gpkg_contents.last_change``, the wall-clock
time of the write to the millisecond, which differs between any two writes of the same layer."""
import os
import sqlite3

import numpy as np
import pytest

import treedetection_amd as T
from treedetection_amd import gpkg
from treedetection_amd import postprocessing as P
from treedetection_amd import treetops as tt
from treedetection_amd.geotiff import write_geotiff

import treetop_cases as tc

pytestmark = pytest.mark.gpu

NAME = "3241"
SCORES = [s for _, s, _ in tc.SCENE_CROWNS]
COUNTS = [n for _, _, n in tc.SCENE_CROWNS]


def _scene(root):
    os.makedirs(root / "img")
    os.makedirs(root / "ndsm")
    pred = root / "out" / "geojson_predictions"
    os.makedirs(pred)
    rgbi = np.zeros((4, 300, 300), np.uint8)
    rgbi[0], rgbi[1], rgbi[2], rgbi[3] = 40, 90, 70, 220     # vegetation everywhere: NDVI about 0.69
    write_geotiff(str(root / "img" / f"{NAME}.tif"), rgbi, tc.IT, 25832, compression="deflate", tile=(128, 128))
    write_geotiff(str(root / "ndsm" / f"{NAME}.tif"), tc.scene_height()[None], tc.HT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    gpkg.write_polygons(str(pred / f"{NAME}.gpkg"), [tc.scene_ring(p) for p, _, _ in tc.SCENE_CROWNS], {"Confidence_score": SCORES}, 25832)
    return pred


class _Log:
    def __getattr__(self, name):
        return lambda m: None


def _config(root, **extra):
    cfg = {"logger": _Log(), "output_directory": str(root / "out"), "height_data_path": str(root / "ndsm"), "image_directory": str(root / "img"),
           "confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 2,
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


def _points(path):
    """The point layer → (srs_id, [(x, y)], columns)"""
    layer = gpkg.read_layer(path)
    return layer.srs_id, [gpkg.parse_point_blob(b)[1] for b in layer.blobs], layer.columns


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("treetops")
    _scene(root)
    off, off_dir = _single(root, "false", crown_treetops=False)
    return root, off, off_dir


def test_absent_and_false_write_the_same_layer_and_nothing_else(scene):
    root, off, off_dir = scene
    absent, absent_dir = _single(root, "absent")
    none, none_dir = _single(root, "none", crown_treetops=None)
    for d in (off_dir, absent_dir, none_dir):
        assert sorted(os.listdir(d)) == [f"processed_{NAME}.gpkg"]
    assert _layer_bytes(absent) == _layer_bytes(off) == _layer_bytes(none)
    rings, cols, _ = gpkg.read_polygons(off)
    assert len(rings) == 5 and cols["Confidence_score"] == SCORES and list(cols) == list(P.COLUMNS)      # the scene keeps all five crowns


def _check_on(root, layer, out, off):
    assert sorted(os.listdir(out)) == [f"processed_{NAME}.gpkg", f"processed_{NAME}_treetops.gpkg"]
    rings, cols, srs = gpkg.read_polygons(layer)
    base_rings, base_cols, _ = gpkg.read_polygons(off)
    assert list(cols) == list(P.COLUMNS) + ["Treetops"] and all(np.array_equal(a, b) for a, b in zip(rings, base_rings))
    assert cols["Treetops"] == COUNTS and all(type(v) is int for v in cols["Treetops"])
    con = sqlite3.connect(layer)
    assert [r[2] for r in con.execute(f'PRAGMA table_info("processed_{NAME}")') if r[1] == "Treetops"] == ["INTEGER"]
    con.close()
    rows_rc = [(r, c) for r, c, _, _ in tc.SCENE_TOPS]
    assert (cols["Treetops"], [o for _, _, _, o in tc.SCENE_TOPS]) == tc.scene_expectation(rings, cols["Confidence_score"], rows_rc)
    srs_id, xy, pc = _points(str(out / f"processed_{NAME}_treetops.gpkg"))
    assert srs_id == srs == 25832 and list(pc) == list(tt.TREETOP_COLUMNS)
    assert list(zip(pc["Row"], pc["Col"])) == rows_rc and pc["Crown"] == [o for _, _, _, o in tc.SCENE_TOPS]
    assert xy == [(tc.HT[2] + c + 0.5, tc.HT[5] - (r + 0.5)) for r, c in rows_rc]
    # the host functions give the same column and the same points
    per_crown, tops = tt.crown_treetops(tc.scene_height(), tc.HT, rings, cols["Confidence_score"], device=None)
    assert per_crown.tolist() == cols["Treetops"] and tops["crown"].tolist() == pc["Crown"]
    assert tops["rows"].tolist() == pc["Row"] and tops["cols"].tolist() == pc["Col"] and [float(v) for v in tops["height"]] == pc["Height"]
    assert all(3.0 < h < spike for h, (_, _, spike, _) in zip(pc["Height"], tc.SCENE_TOPS))
    return cols, pc


def test_the_column_and_the_point_layer_are_as_constructed(scene):
    root, off, _ = scene
    layer, out = _single(root, "true", crown_treetops=True)
    cols, _ = _check_on(root, layer, out, off)
    base = gpkg.read_polygons(off)[1]
    assert all(cols[c] == base[c] for c in P.COLUMNS)


def test_the_height_raster_decoded_in_hbm_is_reused(scene, monkeypatch):
    root, off, _ = scene
    seen = []
    real = P.crown_treetops
    monkeypatch.setattr(P, "crown_treetops", lambda raster, *a, **k: (seen.append(type(raster).__name__), real(raster, *a, **k))[1])
    reads = []
    real_read = P._treetop_raster
    monkeypatch.setattr(P, "_treetop_raster", lambda path, kept, *a: (reads.append(bool(kept.get("full_grid"))), real_read(path, kept, *a))[1])
    layer, out = _single(root, "hbm", crown_treetops=True, device_decode=True)
    _check_on(root, layer, out, off)
    assert seen == ["Tensor"] and reads == [True]


def test_a_scaled_height_raster_is_read_once_more_at_full_size(scene, monkeypatch):
    root, off, _ = scene
    reads = []
    real_read = P._treetop_raster
    monkeypatch.setattr(P, "_treetop_raster", lambda path, kept, *a: (reads.append(bool(kept.get("full_grid"))), real_read(path, kept, *a))[1])
    layer, out = _single(root, "half", crown_treetops=True, height_scaling_factor=0.5)
    assert reads == [False]
    rings, cols, _ = gpkg.read_polygons(layer)
    assert len(rings) == 5 and cols["Treetops"] == COUNTS
    _, _, pc = _points(str(out / f"processed_{NAME}_treetops.gpkg"))
    assert list(zip(pc["Row"], pc["Col"], pc["Crown"])) == [(r, c, o) for r, c, _, o in tc.SCENE_TOPS]


def test_the_parameters_are_read(scene):
    root, off, _ = scene
    layer, out = _single(root, "params", crown_treetops=True, treetop_sigma=0, treetop_window=3, treetop_min_height=11.5)
    cols = gpkg.read_polygons(layer)[1]
    _, _, pc = _points(str(out / f"processed_{NAME}_treetops.gpkg"))
    assert pc["Height"] == [12.0, 13.0, 14.0] and pc["Crown"] == [1, 4, 5] and cols["Treetops"] == [1, 0, 0, 1, 1]     # unsmoothed spikes


def test_a_failure_is_printed_and_keeps_the_layer(scene, monkeypatch, capsys):
    root, off, _ = scene

    def broken(*args, **kw):
        raise RuntimeError("no treetops today")
    monkeypatch.setattr(P, "crown_treetops", broken)
    layer, out = _single(root, "broken", crown_treetops=True)
    printed = capsys.readouterr().out
    assert "Error finding the treetops" in printed and "no treetops today" in printed
    assert sorted(os.listdir(out)) == [f"processed_{NAME}.gpkg"] and _layer_bytes(layer) == _layer_bytes(off)
    monkeypatch.undo()
    monkeypatch.setattr(P, "write_treetops_layer", broken)
    layer, out = _single(root, "unwritten", crown_treetops=True)
    assert "Error writing the treetops" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == [f"processed_{NAME}.gpkg"] and gpkg.read_polygons(layer)[1]["Treetops"] == COUNTS


def test_bad_values_are_refused(scene):
    root, _, _ = scene
    bad = [dict(crown_treetops="yes"), dict(crown_treetops=1), dict(crown_treetops=True, treetop_window=6),
           dict(crown_treetops=True, treetop_window=7.0), dict(crown_treetops=True, treetop_sigma=-1), dict(crown_treetops=True, treetop_sigma="a"),
           dict(crown_treetops=True, treetop_min_height=float("nan"))]
    for k, extra in enumerate(bad):
        with pytest.raises(ValueError, match="crown_treetops must be|treetop_window must be|treetop_sigma must be|treetop_min_height must be"):
            _single(root, f"bad{k}", **extra)
        assert not os.listdir(root / f"bad{k}")


def test_postprocess_files_copies_the_point_layer_next_to_the_layer(tmp_path):
    pred = _scene(tmp_path)
    T.postprocess_files(_config(tmp_path, crown_treetops=True, timestamped_output_directory=True))
    out = tmp_path / "out"
    assert os.path.exists(pred / f"processed_{NAME}_treetops.gpkg") and os.path.exists(out / f"{NAME}.gpkg")
    assert gpkg.read_polygons(str(out / f"{NAME}.gpkg"))[1]["Treetops"] == COUNTS
    _, _, pc = _points(str(out / f"{NAME}_treetops.gpkg"))
    assert list(zip(pc["Row"], pc["Col"], pc["Crown"])) == [(r, c, o) for r, c, _, o in tc.SCENE_TOPS]
    stamped = [d for d in os.listdir(out) if os.path.isdir(out / d) and d not in ("geojson_predictions", "logs")]
    assert len(stamped) == 1 and sorted(os.listdir(out / stamped[0])) == [f"{NAME}.gpkg", f"{NAME}_treetops.gpkg"]
