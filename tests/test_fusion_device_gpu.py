"""``device_outlines``: fuse_predictions and exclude_outlines with the outline predicates on the GPU (Region.relate(device=...),
td_region_relate_dev) write the files they write with the key off — a few hundred crowns of two layers over three parcels, one
with a clearing; an outline in another CRS goes through crs.to_crs on both paths."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from treedetection_amd import gpkg  # noqa: E402
from treedetection_amd.crs import to_crs  # noqa: E402
from treedetection_amd.fusion import exclude_outlines, fuse_predictions, outline_device  # noqa: E402
from treedetection_amd.vector import Region  # noqa: E402

pytestmark = pytest.mark.gpu
ORIGIN = np.array([500000.0, 5600000.0])


def sq(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]], float) + ORIGIN


# three parcels: a block with a clearing, a block sharing an edge with it, one apart
PARCELS = [[sq(100, 100, 200, 200), sq(140, 140, 160, 160)], [sq(200, 100, 260, 200)], [sq(300, 120, 360, 180)]]


def write_outline(path, polygons, epsg):
    feats = [{"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [r.tolist() for r in poly]}} for poly in polygons]
    json.dump({"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": f"urn:ogc:def:crs:EPSG::{epsg}"}}, "features": feats},
              open(path, "w"))


def crowns(seed, n):
    """Star-shaped crowns of 6 - 14 vertices on a 0.25 lattice over the parcels and the ground around them: many straddle a border,
    some touch one exactly."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cx, cy = rng.uniform(80, 380), rng.uniform(80, 220)
        k = int(rng.integers(6, 15))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(1.5, 5.0) * rng.uniform(0.6, 1.0, k)
        ring = np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1) * 4) / 4
        ring = np.concatenate([ring, ring[:1]])
        if abs(np.dot(ring[:-1, 0], ring[1:, 1]) - np.dot(ring[1:, 0], ring[:-1, 1])) > 1:
            out.append(ring + ORIGIN)
    return out


def masked(path):
    """The file's bytes with the writer's time stamp (gpkg_contents.last_change is 'now', a fixed-width text) blanked."""
    return re.sub(rb"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.\d{3}Z", b"<-------- now --------->", open(path, "rb").read())


class Log:
    def __init__(self):
        self.msgs = []

    def __getattr__(self, name):
        return lambda m: self.msgs.append((name, m))


@pytest.fixture(scope="module")
def layers():
    return crowns(1, 300), crowns(2, 300)


@pytest.mark.parametrize("outline_epsg", [25832, 4326], ids=["same CRS", "outline in EPSG:4326"])
def test_fuse_and_exclude_write_the_same_files(tmp_path, layers, outline_epsg, monkeypatch):
    urban_rings, forest_rings = layers
    polygons = PARCELS if outline_epsg == 25832 else to_crs(PARCELS, 25832, outline_epsg)
    outline = str(tmp_path / "forest.geojson")
    write_outline(outline, polygons, outline_epsg)
    lake = str(tmp_path / "lake.geojson")
    write_outline(lake, polygons[:1], outline_epsg)
    used = []
    relate = Region.relate
    monkeypatch.setattr(Region, "relate", lambda self, queries, device=None: (used.append((device, len(queries))), relate(self, queries, device))[1])
    files = {}
    for key in (False, True):
        root = tmp_path / f"key_{key}"
        urban, forest, out = root / "urban_geojson", root / "forrest_geojson", root / "geojson_predictions"
        os.makedirs(urban)
        os.makedirs(forest)
        for folder, rings in ((urban, urban_rings), (forest, forest_rings)):
            gpkg.write_polygons(str(folder / "img1.gpkg"), rings, {"Confidence_score": [0.3 + 0.002 * i for i in range(len(rings))],
                                                                  "filter_index_right": [0] * len(rings)}, 25832)
        config = {"device_outlines": key, "device": "0", "exclude_files": [lake], "output_directory": str(root)}
        log = Log()
        fuse_predictions(str(urban), str(forest), outline, str(out), logger=log, device=outline_device(config))
        assert not [m for m in log.msgs if m[0] == "error"], log.msgs
        fused = masked(out / "img1.gpkg")
        os.rename(out / "img1.gpkg", out / "processed_img1.gpkg")
        exclude_outlines(config, log)
        assert not [m for m in log.msgs if m[0] == "error"], log.msgs
        files[key] = (fused, masked(out / "processed_img1.gpkg"))
    assert [d for d, _ in used] == [None] * 3 + [0] * 3 and [n for _, n in used][:2] == [300, 300]
    assert files[True][0] == files[False][0]                     # the fused layer
    assert files[True][1] == files[False][1]                     # and what the exclusion outline leaves of it
    # the fixture decides something: crowns kept and dropped by both steps
    n_fused = len(gpkg.read_polygons(str(tmp_path / "key_True" / "geojson_predictions" / "processed_img1.gpkg"))[0])
    assert 0 < n_fused < used[2][1] < 600
