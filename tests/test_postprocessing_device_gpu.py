"""The crown stage with both of its rasters on the device path (``device_decode: true``): the four-band uint8 RGBI raster decoded in
HBM, resampled and turned into NDVI there (postprocessing._ndvi_on_device), the float32 nDSM decoded and, at a scaling factor below
one, decimated there (_height_on_device) — process_layer against the host path on a synthetic scene, and the fallback to the host
reader on a corrupt block of the RGBI raster."""
import zlib

import numpy as np
import pytest

from treedetection_amd import postprocessing as P
from treedetection_amd.geotiff import GeoTiff, write_geotiff

from resample_cases import f32_bound

pytestmark = pytest.mark.gpu

SIDE = 600                                                  # RGBI pixels of 0.2 m; the nDSM has SIDE / 5 pixels of 1 m
T = (0.2, 0.0, 412000.0, 0.0, -0.2, 5318120.0)
NT = (1.0, 0.0, 412000.0, 0.0, -1.0, 5318120.0)
RGBI_LAYOUTS = {"lzw": dict(compression="lzw", predictor=2, rows_per_strip=32), "deflate": dict(compression="deflate", tile=(128, 128))}
HEIGHT_THR, NDVI_MEAN_THR, NDVI_VAR_THR = 3.0, 0.2, 0.5


def _scene(seed=21, crowns=36):
    """A four-band uint8 RGBI image with blob crowns (bright or dark in the near-infrared band), an nDSM on a 1 m grid with their
    heights — low crowns up to 2.2 m, tall ones from 5 m — and the crowns' rings with falling scores."""
    rng = np.random.default_rng(seed)
    rgbi = rng.integers(40, 120, (4, SIDE, SIDE), dtype=np.uint8)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    fine = rng.uniform(0, 1.0, (SIDE, SIDE)).astype(np.float32)
    rings = []
    for k in range(crowns):
        cx, cy, r = rng.uniform(40, SIDE - 40), rng.uniform(40, SIDE - 40), rng.uniform(10, 28)
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        inside = d2 < r ** 2
        rgbi[3][inside] = 220 if k % 4 else 60
        hgt = float(rng.uniform(1.2, 2.2) if k % 5 == 0 else rng.uniform(5.0, 25.0))
        fine[inside] = np.maximum(fine[inside], hgt * (1 - d2[inside] / r ** 2 * 0.5))
        ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        ring = np.stack([T[2] + T[0] * (cx + r * np.cos(ang)), T[5] + T[4] * (cy + r * np.sin(ang))], axis=1)
        rings.append(np.concatenate([ring, ring[:1]]))
    ndsm = fine.reshape(SIDE // 5, 5, SIDE // 5, 5).max(axis=(1, 3)).astype(np.float32)
    scores = [0.97 - 0.015 * k for k in range(crowns)]
    return rgbi, ndsm, rings, scores


def _config(device_decode, n_scale, h_scale):
    return {"confidence_threshold": 0.3, "iou_threshold": 0.5, "area_threshold": 1, "containment_threshold": 0.9, "height_threshold": HEIGHT_THR,
            "ndvi_mean_threshold": NDVI_MEAN_THR, "ndvi_var_threshold": NDVI_VAR_THR, "use_overlap": False, "tile_width": 50, "tile_height": 50,
            "buffer": 10, "overlapping_tiles_width": 3, "overlapping_tiles_height": 3, "ndvi_scaling_factor": n_scale,
            "height_scaling_factor": h_scale, "device_decode": device_decode}


def _same_features(a, b, height_tol=0.0):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa["ring"], fb["ring"]) and fa["properties"].keys() == fb["properties"].keys()
        for k, v in fa["properties"].items():
            w = fb["properties"][k]
            if k == "TreeHeight" and height_tol:
                assert abs(v - w) <= height_tol, (k, v, w)
            else:
                assert (np.float64(v).tobytes() == np.float64(w).tobytes()) if isinstance(v, float) else v == w, k


@pytest.fixture
def stats(monkeypatch):
    """Records what crown_stats returns, per call, while process_layer runs."""
    seen = []
    real = P.crown_stats

    def recording(*args, **kw):
        out = real(*args, **kw)
        seen.append((args[4], out))                         # (mode, statistics)
        return out
    monkeypatch.setattr(P, "crown_stats", recording)
    return seen


def _assert_clear_of_the_thresholds(seen):
    """No crown's statistic lies within 1e-3 of the threshold it is compared with: the selection cannot hinge on the last bits."""
    assert seen
    for mode, out in seen:
        if mode == 0:
            assert (np.abs(out[:, 0] - HEIGHT_THR) > 1e-3).all()
        else:
            assert (np.abs(out[:, 2] - NDVI_MEAN_THR) > 1e-3).all() and (np.abs(out[:, 3] - NDVI_VAR_THR) > 1e-3).all()


def _no_host_reader(self):
    raise AssertionError(f"{self.path} went through the host reader")


@pytest.mark.parametrize("layout", sorted(RGBI_LAYOUTS))
def test_process_layer_is_the_same_on_both_paths(tmp_path, monkeypatch, stats, layout):
    rgbi, ndsm, rings, scores = _scene()
    rpath, hpath = str(tmp_path / "rgbi.tif"), str(tmp_path / "ndsm.tif")
    write_geotiff(rpath, rgbi, T, 25832, **RGBI_LAYOUTS[layout])
    write_geotiff(hpath, ndsm[None], NT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    assert GeoTiff(rpath).device_decodable() and GeoTiff(hpath).device_decodable(float_samples=True)
    bound = f32_bound(ndsm.shape[0], ndsm.shape[1], ndsm.shape[0] // 2, ndsm.shape[1] // 2, np.abs(ndsm).max())
    for h_scale, tol in ((1.0, 0.0), (0.5, bound)):
        del stats[:]
        host = P.process_layer(rings, scores, _config(False, 0.2, h_scale), hpath, rpath)
        _assert_clear_of_the_thresholds(stats)
        with monkeypatch.context() as m:
            m.setattr(GeoTiff, "read", _no_host_reader)     # neither raster may take the host route
            dev = P.process_layer(rings, scores, _config(True, 0.2, h_scale), hpath, rpath)
        _assert_clear_of_the_thresholds(stats)
        heights = [f["properties"]["TreeHeight"] for f in host]
        print(f"{layout}, height factor {h_scale}: {len(host)} features, TreeHeight {min(heights):.2f} .. {max(heights):.2f}, tolerance {tol:.3e}")
        assert len(host) >= 12 and len(host) < len(rings)   # the thresholds select: some crowns stay, some go
        _same_features(host, dev, tol)
    # "auto" and an absent key keep the host reader for both rasters
    host = P.process_layer(rings, scores, _config(False, 0.2, 1.0), hpath, rpath)
    cfg = _config("auto", 0.2, 1.0)
    with monkeypatch.context() as m:
        m.setattr(P, "resample_on_device", lambda *a, **k: pytest.fail("the device path ran"))
        _same_features(host, P.process_layer(rings, scores, cfg, hpath, rpath))
        del cfg["device_decode"]
        _same_features(host, P.process_layer(rings, scores, cfg, hpath, rpath))


def _outcome(fn):
    try:
        return ("features", fn())
    except Exception as e:                                  # noqa: BLE001 — the outcome IS the exception when the host reader raises
        return ("raised", type(e).__name__, str(e))


def test_a_corrupt_rgbi_block_falls_back_to_the_host_reader(tmp_path, capsys):
    """One bit of block 1's Adler-32 trailer flipped in the DEFLATE RGBI raster: the device path prints the block and the fallback line
    and process_layer returns what the host path returns — here zlib's own "incorrect data check", exactly as with the device path off."""
    rgbi, ndsm, rings, scores = _scene()
    good, bad, hpath = str(tmp_path / "good.tif"), str(tmp_path / "bad.tif"), str(tmp_path / "ndsm.tif")
    write_geotiff(good, rgbi, T, 25832, **RGBI_LAYOUTS["deflate"])
    write_geotiff(hpath, ndsm[None], NT, 25832, compression="deflate", predictor=3, tile=(32, 32))
    g = GeoTiff(good)
    g._setup_blocks()
    off, cnt = int(g._offs[1]), int(g._counts[1])
    g.close()
    raw = bytearray(open(good, "rb").read())
    raw[off + cnt - 2] ^= 0x10
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(zlib.error, match="incorrect data check"):
        zlib.decompress(bytes(raw[off:off + cnt]))
    capsys.readouterr()
    host = _outcome(lambda: P.process_layer(rings, scores, _config(False, 0.2, 1.0), hpath, bad))
    assert "using the host reader" not in capsys.readouterr().out
    dev = _outcome(lambda: P.process_layer(rings, scores, _config(True, 0.2, 1.0), hpath, bad))
    log = capsys.readouterr().out
    assert "block 1: Adler-32 mismatch" in log and f"device decode of {bad} failed" in log and "using the host reader" in log
    assert host[0] == "raised" and "incorrect data check" in host[2] and dev == host
    _same_features(P.process_layer(rings, scores, _config(False, 0.2, 1.0), hpath, good), P.process_layer(rings, scores, _config(True, 0.2, 1.0), hpath, good))
