"""The engine's two profile books (td_engine_profile_read: FLOPs, bytes and layers per category; td_engine_profile_classes: executed
FLOPs, moved bytes and t_min per speed-of-light class) of ONE forward, case by case against figures recorded once, by the commit named
in each file of tests/golden/profile_books. bench.py derives its MFU and speed-of-light shares from these books, and every launch
form books by its own formula (csrc/launch_cost.h), so each case switches the forward onto other forms: B = 2 at 128 x 160 on the
full-width R50 (pyramid 32x40, 16x20, 8x10, 4x5, 2x3: p2 and p3 take F(4x4), the rest F(2x2)).

No case's books depend on which tile the tuner picked. The one site where they would is HEAD_IF_TILE_OWNS_256 (fp16, levels not
grouped, head fusion on): the ungrouped fp16 case turns head fusion off, and the default fp16 engine runs the RPN as the grouped launch,
which asks conv_path nothing. So the engine's run_conv meets every ConvForm and HEAD_IN_TRANSFORM in these cases, and never
HEAD_IF_TILE_OWNS_256 (test_the_cases_reach_every_form: host only)."""
import json
import os

import numpy as np
import pytest

from treedetection_amd import _lib
from treedetection_amd.weights import make_synthetic_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_books")
B, H, W = 2, 128, 160
SIDES = ((32, 40), (16, 20), (8, 10), (4, 5), (2, 3))          # p2 .. p6
D = 100                                                          # detections per image: the mask head reserves B * D RoIs

# name -> (precision, switches read at engine creation, profile mode)
CASES = {
    "fp32_defaults": ("fp32", {}, 1),
    "fp32_defaults_detail": ("fp32", {}, 2),
    "fp32_wino_fold_55": ("fp32", {"TD_WINO_FOLD": "55"}, 1),
    "fp32_wino_fused_0": ("fp32", {"TD_WINO_FUSED": "0"}, 1),
    "fp32_fuse_tail_0": ("fp32", {"TD_FUSE_TAIL": "0"}, 1),
    "fp32_no_split": ("fp32", {"TD_F32_SPLIT": "0", "TD_F32_SPLIT_TAIL": "0", "TD_F32_SPLIT_WINO": "0"}, 1),
    "fp32_fuse_head_0": ("fp32", {"TD_FUSE_HEAD": "0"}, 1),
    "fp32_backbone_subbatch_1": ("fp32", {"TD_BACKBONE_SUBBATCH": "1"}, 1),
    "fp16_defaults": ("fp16", {}, 1),
    "fp16_ungrouped_fuse_head_0": ("fp16", {"TD_GROUP_LEVELS": "0", "TD_FUSE_HEAD": "0"}, 1),
    "fp16_fuse_tail_2": ("fp16", {"TD_FUSE_TAIL": "2"}, 1),
}


def inputs():
    rng = np.random.default_rng(11)
    return [{"image": rng.integers(0, 256, (3, H, W)).astype(np.float32), "height": H, "width": W} for _ in range(B)]


def measure(sd, precision, mode):
    """One tuning / warm-up forward, then the books of one profiled forward (the switches of the case are in the environment)."""
    from treedetection_amd.engine import Engine
    eng = Engine(sd, device=0, precision=precision)
    try:
        x = inputs()
        eng(x)
        eng.profile_enable(mode)
        eng.profile_read(reset=True)
        eng.profile_classes(reset=True)
        eng(x)
        return {"categories": eng.profile_read(), "classes": eng.profile_classes()}
    finally:
        eng.close()


@pytest.fixture(scope="module")
def sd():
    return make_synthetic_state_dict(50, seed=3)


@pytest.fixture(scope="module")
def tune_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("books") / "tune.txt")


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b)) if max(abs(a), abs(b)) > 0 else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_books_equal_the_recorded_ones(name, sd, tune_cache, monkeypatch):
    precision, env, mode = CASES[name]
    want = json.load(open(os.path.join(GOLDEN, name + ".json")))
    assert want["switches"] == env and want["precision"] == precision and len(want["commit"]) == 40
    monkeypatch.setenv("TD_TUNE_CACHE", tune_cache)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = measure(sd, precision, mode)
    for book, sums in (("categories", ("flops", "bytes")), ("classes", ("exec_flops", "bytes", "tmin_ms"))):
        assert got[book].keys() == want[book].keys()
        for k, w in want[book].items():
            g = got[book][k]
            print(name, book, k, g, w)
            assert g["launches"] == w["launches"], (book, k)
            # regrouped sums of a few hundred non-negative doubles move by ~1e-13 at the most; more is another formula
            for f in sums:
                assert rel(g[f], w[f]) <= 1e-12, (book, k, f, g[f], w[f])
        # every bracket still records its events: the same rows carry a time (classes: in detail mode only)
        assert {k for k, g in got[book].items() if g["ms"] > 0} == {k for k, w in want[book].items() if w["ms"] > 0}, book
    assert any(w["ms"] > 0 for w in want["classes"].values()) == (mode == 2)


# ---- host only: which forms the sites of the cases take -------------------------------------------------------------------------
def layer(cout, cin, k, scale=0, out_f32=0, banks=""):
    return [cout, cin, k, k, scale, out_f32, "2" in banks, "4" in banks, "s" in banks]


def sites(precision, split):
    """The run_conv sites of the forward above that can leave the direct form, with the banks the loader gives their layers."""
    s = "s" if split and precision == 0 else ""
    w = "24" if precision == 0 else ""
    call = lambda hw, **kw: [kw.get("B", B), hw[0], hw[1], 1, kw.get("pad", 1), kw.get("relu", 1), kw.get("res", 0), 0, kw.get("dyn", 0), kw.get("mul", 1)]
    out = [(layer(128, 128, 3, scale=1, banks=w), call(SIDES[1]), None),                                       # res3 conv2
           (layer(256, 256, 3, scale=1, banks=w + s), call(SIDES[2]), None),                                   # res4 conv2
           (layer(256, 1024, 1, banks=s), call(SIDES[2], pad=0, relu=0, res=1), None),                         # fpn_lateral4
           (layer(1024, 12544, 1, banks=s), call((1, 1), B=B * 1000, pad=0), None),                            # fc1
           (layer(256, 256, 3, banks=w), call((14, 14), B=B * D, dyn=1, mul=196), None)]                       # mask_fcn
    for hw in SIDES:
        out.append((layer(256, 256, 3, banks=w + s), call(hw), layer(15, 256, 1, out_f32=1)))                 # rpn conv + head
        out.append((layer(256, 256, 3, banks=w + s), call(hw, relu=0), None))                                  # fpn_output
    return out


def test_the_cases_reach_every_form(monkeypatch):
    mid = [64, 128, 256, 512]
    widths = [64] + mid + mid + [4 * m for m in mid] + [256, 1024, 256]
    forms, heads = set(), set()
    for name, (precision, env, _) in CASES.items():
        for k in ("TD_WINO_FOLD", "TD_WINO_FUSED", "TD_FUSE_HEAD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)                     # td_conv_path reads the rule switches as an engine created now would
        prec = {"fp32": 0, "fp16": 1}[precision]
        plan = {r["name"]: r["alloc_bytes"] for r in _lib.workspace_plan(prec, 1, 1000, D, widths, B, H, W)}
        grouped = prec == 1 and env.get("TD_GROUP_LEVELS") != "0"
        for lay, call, head in sites(prec, env.get("TD_F32_SPLIT") != "0"):
            if grouped and lay[:3] == [256, 256, 3] and not call[8]:
                continue                                 # the grouped launch: run_grouped asks conv_path nothing
            got = _lib.conv_path([prec] + [-1] * 7, plan.get("wino_v", 0) // 4, lay, call, head)
            forms.add(got["form"])
            heads.add(got["head"])
    assert forms == set(_lib.CONV_FORMS)
    assert heads == {_lib.CONV_HEADS[0], _lib.CONV_HEADS[1]}
