"""The engine's workspace plan (csrc/workspace.cpp) through its host-only entry td_workspace_plan: the public rows against what
td_engine_tensor replied before the plan existed (tests/golden/engine_tensors.json, recorded on the GPU after full forwards),
every allocation against a restatement of the hand-written td_engine_reserve the table replaced, and the property nothing checked
then: whatever shape a forward publishes fits the allocation of every reservation that covers it. Host only."""
import json
import os
from math import prod

import pytest

from treedetection_amd import _lib

FP32, FP16 = 0, 1
P, D = 1000, 100                       # td_model_desc_default: post_nms_topk, detections_per_image
SHAPE_A, SHAPE_B = (2, 256, 320), (1, 160, 224)          # (b): p5 is 5 x 7, odd on both axes, so p6 rounds up to 3 x 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_tensors.json")


def widths(width_div):
    """What the loader reads off make_synthetic_state_dict(50, width_div=...): stem; conv1, conv2, conv3 of res2 .. res5; FPN; FC;
    mask deconv output."""
    mid = [64, 128, 256, 512]
    return [c // width_div for c in [64] + mid + mid + [4 * m for m in mid] + [256, 1024, 256]]


def plan(precision, width_div, shape, winograd=1):
    return _lib.workspace_plan(precision, winograd, P, D, widths(width_div), *shape)


def parent_reserve(precision, winograd, wd, B, Hp, Wp):
    """td_engine_reserve as it was written by hand before the table, one entry per hipMalloc, in bytes (from its source:
    `A(&e->x, elems)` allocates elems * sizeof(*e->x), `AA` elems * the activation size)."""
    w = widths(wd)
    stem_c, c1, c2, c3, fpn_c, fc_dim, deconv_q = w[0], w[1:5], w[5:9], w[9:13], w[13], w[14], w[15]
    es = 2 if precision == FP16 else 4
    f32 = i32 = u32 = 4
    u64 = 8
    out = {}
    out["stem_out"] = B * (Hp // 2) * (Wp // 2) * stem_c * es
    out["pool_out"] = B * (Hp // 4) * (Wp // 4) * stem_c * es
    hs = [Hp >> (l + 2) for l in range(4)]
    ws = [Wp >> (l + 2) for l in range(4)]
    hs.append((hs[3] - 1) // 2 + 1)
    ws.append((ws[3] - 1) // 2 + 1)
    for s in range(4):
        px = B * hs[s] * ws[s]
        out[f"t1[{s}]"] = px * c1[s] * es
        out[f"t2[{s}]"] = px * c1[s] * es
        out[f"scb[{s}]"] = px * c3[s] * es
        out[f"res[{s}]"] = px * c3[s] * es
        out[f"xtmp[{s}]"] = px * c3[s] * es
        out[f"inner[{s}]"] = px * fpn_c * es
    total_anchors = 0
    for l in range(5):
        px = B * hs[l] * ws[l]
        out[f"pfeat[{l}]"] = px * fpn_c * es
        out[f"rpn_headbuf[{l}]"] = px * 15 * f32
        total_anchors += hs[l] * ws[l] * 3
    out["rpn_t"] = B * hs[0] * ws[0] * fpn_c * es
    out["key_ws"] = B * (total_anchors + 5 * 4096) * u32          # rpn_topk_ws_elems: dense keys + 5 histograms of 1 << 12 bins per image
    nc = B * 5 * 1024
    out["cand_boxes"] = nc * 4 * f32
    out["cand_scores"] = nc * f32
    out["cand_valid"] = nc * i32
    out["cand_idx"] = nc * i32
    out["nms_mask"] = nc * (1024 // 64) * u64
    out["rpn_keep"] = nc * i32
    out["rpn_keep_count"] = B * 5 * i32
    out["props"] = B * P * 4 * f32
    out["prop_scores"] = B * P * f32
    out["prop_count"] = B * i32
    out["pooled7"] = B * P * 49 * fpn_c * es
    out["fc1_out"] = B * P * fc_dim * es
    out["fc2_out"] = B * P * fc_dim * es
    out["pred_out"] = B * P * 6 * f32
    out["dboxes"] = B * P * 4 * f32
    out["dscores"] = B * P * f32
    out["dflags"] = B * P * i32
    out["sboxes"] = B * P * 4 * f32
    out["sscores"] = B * P * f32
    out["sidx"] = B * P * i32
    out["scount"] = B * i32
    out["det_keep"] = B * D * i32
    out["det_keep_count"] = B * i32
    out["det_boxes_net"] = B * D * 4 * f32
    mrows = B * D
    out["pooled14"] = mrows * 196 * fpn_c * es
    out["mbuf0"] = mrows * 196 * fpn_c * es
    out["mbuf1"] = mrows * 196 * fpn_c * es
    out["deconv_out"] = mrows * 784 * deconv_q * es
    out["mask_logits"] = mrows * 784 * f32
    out["mask_probs_compact"] = mrows * 784 * f32
    out["total_rows"] = 4 * i32
    out["o_boxes"] = B * D * 4 * f32
    out["o_scores"] = B * D * f32
    out["o_classes"] = B * D * i32
    out["o_count"] = B * i32
    out["o_mask_probs"] = mrows * 784 * f32
    if precision == FP32 and winograd:
        tiles = lambda h, w_: ((h + 1) // 2) * ((w_ + 1) // 2)
        need = 0
        for l in range(5):
            need = max(need, B * tiles(hs[l], ws[l]) * fpn_c)
        for s in range(4):
            need = max(need, B * tiles(hs[s], ws[s]) * c2[s])
        need = max(need, mrows * tiles(14, 14) * fpn_c)
        out["wino_v"] = 16 * need * f32
        out["wino_m"] = 16 * need * f32
    return out


with open(GOLDEN) as f:
    RECORDED = json.load(f)


def test_the_recording_holds_the_four_configurations():
    """fp32 and fp16 engines at shapes (a) and (b). The fp32 engine ran make_synthetic_state_dict(50, seed=3, width_div=2); the fp16
    engine ran it at full width, because its kernels contract 64-channel chunks and refuse the 32-channel res2 of width_div=2."""
    got = {k: (v["precision"], v["width_div"], (v["B"], v["Hp"], v["Wp"])) for k, v in RECORDED.items()}
    assert got == {"fp32/a": ("fp32", 2, SHAPE_A), "fp32/b": ("fp32", 2, SHAPE_B), "fp16/a": ("fp16", 1, SHAPE_A), "fp16/b": ("fp16", 1, SHAPE_B)}
    assert all(len(v["tensors"]) == 43 for v in RECORDED.values())


@pytest.mark.parametrize("key", sorted(RECORDED))
def test_public_rows_equal_the_recorded_replies(key):
    rec = RECORDED[key]
    rows = plan({"fp32": FP32, "fp16": FP16}[rec["precision"]], rec["width_div"], (rec["B"], rec["Hp"], rec["Wp"]))
    got = {r["public"]: {"dims": r["dims"], "elem": r["elem"]} for r in rows if r["public"]}
    assert sorted(got) == sorted(rec["tensors"])           # no name missing, none extra
    assert got == rec["tensors"]


@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B, (8, 800, 800)])
@pytest.mark.parametrize("winograd", [0, 1])
@pytest.mark.parametrize("width_div", [1, 2])
@pytest.mark.parametrize("precision", [FP32, FP16])
def test_allocations_equal_the_hand_written_reserve(precision, width_div, winograd, shape):
    want = parent_reserve(precision, winograd, width_div, *shape)
    rows = plan(precision, width_div, shape, winograd)
    assert len(rows) == len(want) == (76 if precision == FP32 and winograd else 74)      # one hipMalloc each, as many as before
    assert {r["name"]: r["alloc_bytes"] for r in rows} == want


SIDES = range(64, 257, 32)


def test_what_a_forward_publishes_fits_every_reservation_that_covers_it():
    """product(extents) x elem of every public row at (B, Hp, Wp) <= its allocation at any (B', Hp', Wp') >= it: td_engine_reserve
    sizes for the largest shape, forwards of smaller batches publish (and stage tests read and write) their own extents."""
    for precision, wd in ((FP32, 2), (FP16, 1)):
        plans = {(B, Hp, Wp): {r["public"]: r for r in plan(precision, wd, (B, Hp, Wp)) if r["public"]}
                 for B in (1, 2, 3) for Hp in SIDES for Wp in SIDES}
        used = {k: {n: prod(d for d in r["dims"] if d > 0) * r["elem"] for n, r in v.items()} for k, v in plans.items()}
        for (B, Hp, Wp), small in used.items():
            for (B2, Hp2, Wp2), big in plans.items():
                if B2 >= B and Hp2 >= Hp and Wp2 >= Wp:
                    for name, nbytes in small.items():
                        assert nbytes <= big[name]["alloc_bytes"], (name, (B, Hp, Wp), (B2, Hp2, Wp2))


@pytest.mark.parametrize("precision,wd", [(FP32, 2), (FP16, 1)])
def test_public_rows_are_well_formed(precision, wd):
    rows = [r for r in plan(precision, wd, SHAPE_B) if r["public"]]
    names = [r["public"] for r in rows]
    assert len(names) == len(set(names)) == 43
    for r in rows:
        assert r["phase"] in range(7), r
        assert any(d > 0 for d in r["dims"]), r
        assert r["elem"] == ((2 if precision == FP16 else 4) if r["kind"] == "act" else 4), r
    assert {r["public"] for r in rows if r["phase"] == 6} == {"stem", "pool"}


def test_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.td_workspace_plan(0, 1, P, D, None, 1, 64, 64, None, 0, None) == _lib.ERR_INVALID
    with pytest.raises(_lib.TdError):
        plan(FP32, 2, (1, 100, 64))                        # padded sizes are multiples of 32
    with pytest.raises(_lib.TdError):
        _lib.workspace_plan(FP32, 1, 2000, D, widths(1), 1, 64, 64)
