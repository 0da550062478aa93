"""``crown_treetops`` without a GPU: the host functions (``device=None``) on the scene of tests/treetop_cases.py — treetops per crown
2, 1, 0, 1, 2 and the owner of every treetop as constructed and as an even-odd test over the pixel centres says —, treetops_file
and the command line on a written GeoTIFF, the config keys, the resume parameters, and which layers the exclude filter reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

import treetop_cases as tc
from treedetection_amd import gpkg
from treedetection_amd import postprocessing as P
from treedetection_amd import treetops as tt
from treedetection_amd.geotiff import write_geotiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [tc.scene_ring(p) for p, _, _ in tc.SCENE_CROWNS]
SCORES = [s for _, s, _ in tc.SCENE_CROWNS]
TOPS_RC = [(r, c) for r, c, _, _ in tc.SCENE_TOPS]


def test_host_functions_count_and_name_as_constructed():
    per_crown, tops = tt.crown_treetops(tc.scene_height(), tc.HT, RINGS, SCORES, device=None)
    assert per_crown.dtype == np.int64 and per_crown.tolist() == [n for _, _, n in tc.SCENE_CROWNS]
    assert list(zip(tops["rows"].tolist(), tops["cols"].tolist())) == TOPS_RC
    assert tops["crown"].tolist() == [o for _, _, _, o in tc.SCENE_TOPS]
    assert (per_crown.tolist(), tops["crown"].tolist()) == tc.scene_expectation(RINGS, SCORES, TOPS_RC)
    assert tops["xy"].tolist() == [[tc.HT[2] + c + 0.5, tc.HT[5] - (r + 0.5)] for r, c in TOPS_RC]
    smoothed = tc.oracle(tc.scene_height(), tc.weights(0.5), 7, 3.0)[1]
    assert tc.same_floats(tops["height"], smoothed[tops["rows"], tops["cols"]])


def test_equal_scores_go_to_the_lower_index_and_order_does_not_matter():
    # every top under two copies of every crown: the first copy owns it; reversed, the counts follow the rings
    per_crown, tops = tt.crown_treetops(tc.scene_height(), tc.HT, RINGS + RINGS, SCORES + SCORES, device=None)
    assert per_crown.tolist() == 2 * [n for _, _, n in tc.SCENE_CROWNS] and tops["crown"].tolist() == [o for _, _, _, o in tc.SCENE_TOPS]
    per_crown, tops = tt.crown_treetops(tc.scene_height(), tc.HT, RINGS[::-1], SCORES[::-1], device=None)
    assert (per_crown.tolist(), tops["crown"].tolist()) == tc.scene_expectation(RINGS[::-1], SCORES[::-1], TOPS_RC)
    assert per_crown.tolist() == [n for _, _, n in tc.SCENE_CROWNS][::-1]


def test_no_crowns_and_no_tops():
    per_crown, tops = tt.crown_treetops(tc.scene_height(), tc.HT, [], [], device=None)
    assert per_crown.shape == (0,) and tops["crown"].tolist() == [0] * 6
    per_crown, tops = tt.crown_treetops(np.zeros((60, 60), np.float32), tc.HT, RINGS, SCORES, device=None)
    assert per_crown.tolist() == [0] * 5 and tops["rows"].size == 0 and tops["xy"].shape == (0, 2)
    degenerate = [RINGS[0], RINGS[0][:2]]                                               # a ring of one edge is refused: it counts nothing
    assert tt.crown_treetops(tc.scene_height(), tc.HT, degenerate, [0.9, 0.8], device=None)[0].tolist() == [2, 0]


def test_treetops_file_and_the_command_line(tmp_path):
    path, out = str(tmp_path / "ndsm.tif"), str(tmp_path / "tops.gpkg")
    write_geotiff(path, tc.scene_height()[None], tc.HT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    assert tt.treetops_file(path, out, device=None) == 6
    layer = gpkg.read_layer(out)
    assert layer.srs_id == 25832 and list(layer.columns) == list(tt.TREETOP_COLUMNS) and layer.columns["Crown"] == [0] * 6
    assert list(zip(layer.columns["Row"], layer.columns["Col"])) == TOPS_RC
    assert [gpkg.parse_point_blob(b)[1] for b in layer.blobs] == [(tc.HT[2] + c + 0.5, tc.HT[5] - (r + 0.5)) for r, c in TOPS_RC]
    cli = str(tmp_path / "cli.gpkg")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "treetops.py"), path, cli, "--host", "--sigma", "0", "--window", "3",
                        "--min-height", "11.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "3 treetop(s)" in r.stdout, r.stdout + r.stderr
    assert gpkg.read_layer(cli).columns["Height"] == [12.0, 13.0, 14.0]


def test_the_config_keys():
    assert P.crown_treetops_setting({}) is None and P.crown_treetops_setting({"crown_treetops": None}) is None
    assert P.crown_treetops_setting({"crown_treetops": False, "treetop_window": 6}) is None            # (off: the parameters are not read)
    assert P.crown_treetops_setting({"crown_treetops": True}) == {"sigma": 0.5, "window": 7, "min_height": 3.0}
    assert P.crown_treetops_setting({"crown_treetops": True, "treetop_sigma": 1, "treetop_window": 9, "treetop_min_height": 2}) == \
        {"sigma": 1.0, "window": 9, "min_height": 2.0}
    assert P.crown_treetops_setting({"crown_treetops": True, "treetop_sigma": None, "treetop_min_height": float("-inf")})["min_height"] == float("-inf")
    for bad in ({"crown_treetops": "true"}, {"crown_treetops": 1}, {"crown_treetops": True, "treetop_window": 8},
                {"crown_treetops": True, "treetop_window": 0}, {"crown_treetops": True, "treetop_window": True},
                {"crown_treetops": True, "treetop_sigma": float("inf")}, {"crown_treetops": True, "treetop_sigma": -0.5},
                {"crown_treetops": True, "treetop_min_height": float("nan")}, {"crown_treetops": True, "treetop_min_height": "3"}):
        with pytest.raises(ValueError):
            P.crown_treetops_setting(bad)
    import yaml
    with open(os.path.join(ROOT, "example", "config.yml")) as f:
        cfg = yaml.safe_load(f)
    assert (cfg["crown_treetops"], cfg["treetop_sigma"], cfg["treetop_window"], cfg["treetop_min_height"]) == (False, 0.5, 7, 3.0)
    assert P.crown_treetops_setting(cfg) is None
    assert P.crown_treetops_setting(dict(cfg, crown_treetops=True)) == {"sigma": 0.5, "window": 7, "min_height": 3.0}


def test_the_resume_file_knows_the_key(tmp_path):
    base = {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": 3,
            "tile_width": 50, "tile_height": 50, "buffer": 10, "confidence_threshold_stitching": 0.3}
    off, _ = P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_treetops=False))
    plain, _ = P.load_recovery_data_with_params(str(tmp_path), base)
    on, _ = P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_treetops=True, treetop_window=9))
    assert off == plain and "crown_treetops" not in off and on["crown_treetops"] == {"sigma": 0.5, "window": 9, "min_height": 3.0}
    P.save_recovery_data_with_params(str(tmp_path), plain, ["a.gpkg"])
    assert P.load_recovery_data_with_params(str(tmp_path), base)[1] == {"a.gpkg"}
    assert P.load_recovery_data_with_params(str(tmp_path), dict(base, crown_treetops=True))[1] == set()      # layers without the column are not done


def test_the_exclude_filter_leaves_the_point_layer_alone(tmp_path):
    from treedetection_amd.fusion import exclude_outlines
    pred = tmp_path / "geojson_predictions"
    os.makedirs(pred)
    gpkg.write_polygons(str(pred / "processed_a.gpkg"), RINGS, {"Confidence_score": SCORES}, 25832)
    _, tops = tt.crown_treetops(tc.scene_height(), tc.HT, RINGS, SCORES, device=None)
    tt.write_treetops_layer(str(pred / "processed_a_treetops.gpkg"), tops, 25832)
    before = open(pred / "processed_a_treetops.gpkg", "rb").read()
    gpkg.write_polygons(str(tmp_path / "exclude.gpkg"), [tc.scene_ring([(0, 0), (30, 0), (30, 30), (0, 30)])], {}, 25832)
    exclude_outlines({"output_directory": str(tmp_path), "exclude_files": [str(tmp_path / "exclude.gpkg")]})
    assert len(gpkg.read_layer(str(pred / "processed_a.gpkg"))) < 5
    assert open(pred / "processed_a_treetops.gpkg", "rb").read() == before
