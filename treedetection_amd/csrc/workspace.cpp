// The engine's workspace plan (workspace.h): the geometry, the table of buffers, and td_workspace_plan, which reads the table out.
#include "workspace.h"
#include "detect.h"

#include <algorithm>
#include <cstdio>

WsGeom ws_geom(int precision, bool winograd, int P, int D, const int32_t widths[WS_WIDTHS], int B, int Hp, int Wp) {
    WsGeom g{};
    g.B = B; g.Hp = Hp; g.Wp = Wp; g.P = P; g.D = D; g.mrows = B * D;
    auto side = [](int padded, int l) { return padded >> (l + 2); };      // p2 .. p5: strides 4 .. 32
    for (int l = 0; l < 4; ++l) { g.h[l] = side(Hp, l); g.w[l] = side(Wp, l); }
    g.h[4] = (g.h[3] - 1) / 2 + 1; g.w[4] = (g.w[3] - 1) / 2 + 1;       // p6: p5 subsampled with stride 2 (an odd side rounds up)
    for (int l = 0; l < 5; ++l) g.total_anchors += g.h[l] * g.w[l] * RPN_A;
    g.es = precision == TD_PRECISION_FP16 ? 2 : 4;
    g.wino = precision == TD_PRECISION_FP32 && winograd;
    for (int s = 0; s < 4; ++s) { g.c1[s] = widths[1 + s]; g.c2[s] = widths[5 + s]; g.c3[s] = widths[9 + s]; }
    g.stem_c = widths[0]; g.fpn_c = widths[13]; g.fc_dim = widths[14]; g.deconv_q = widths[15];
    return g;
}

// Winograd workspace: 16 planes of [tiles][channels] for V and for M of the largest 3x3 layer that takes the path (FPN / RPN at
// p2, the bottleneck conv2 of every stage, the mask head over B*D RoIs of 14x14)
size_t ws_wino_elems(const WsGeom& g) {
    if (!g.wino) return 0;
    auto tiles = [](int h, int w) { return (size_t)((h + 1) / 2) * ((w + 1) / 2); };
    size_t need = (size_t)g.mrows * tiles(14, 14) * (size_t)g.fpn_c;
    for (int l = 0; l < 5; ++l) need = std::max(need, (size_t)g.B * tiles(g.h[l], g.w[l]) * (size_t)g.fpn_c);
    for (int s = 0; s < 4; ++s) need = std::max(need, (size_t)g.B * tiles(g.h[s], g.w[s]) * (size_t)g.c2[s]);
    return 16 * need;
}

#define AT(m) #m, offsetof(Workspace, m), (int)(sizeof(Workspace::m) / sizeof(void*))
#define DIMS(...) [](const WsGeom& g, int i) -> WsDims { (void)i; return {{__VA_ARGS__}}; }
#define ELEMS(x) [](const WsGeom& g) -> size_t { return x; }
constexpr int L = RPN_LEVELS, K = RPN_CAND, NONE = -1;

const std::vector<WsRow>& ws_rows() {
    static const std::vector<WsRow> rows = {
        // member, kind, extents, allocation (elements) where it is not their product, public name, phase
        {AT(stem_out), WS_ACT, DIMS(g.B, g.Hp / 2, g.Wp / 2, g.stem_c), nullptr, "stem", TD_PHASE_STEM},
        {AT(pool_out), WS_ACT, DIMS(g.B, g.Hp / 4, g.Wp / 4, g.stem_c), nullptr, "pool", TD_PHASE_STEM},
        {AT(t1), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.c1[i]), nullptr, nullptr, NONE},
        {AT(t2), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.c1[i]), nullptr, nullptr, NONE},      // (conv2 keeps conv1's width)
        {AT(scb), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.c3[i]), nullptr, nullptr, NONE},
        {AT(res), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.c3[i]), nullptr, "res%d", 0},
        {AT(xtmp), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.c3[i]), nullptr, nullptr, NONE},
        {AT(inner), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.fpn_c), nullptr, nullptr, NONE},
        {AT(pfeat), WS_ACT, DIMS(g.B, g.h[i], g.w[i], g.fpn_c), nullptr, "p%d", 0},
        {AT(rpn_headbuf), WS_F32, DIMS(g.B, g.h[i], g.w[i], RPN_HEAD_C), nullptr, "rpn_head%d", 0},
        {AT(rpn_t), WS_ACT, DIMS(g.B, g.h[0], g.w[0], g.fpn_c), nullptr, nullptr, NONE},    // one level at a time: sized for p2, the largest
        {AT(key_ws), WS_U32, DIMS(g.B, g.total_anchors), ELEMS(rpn_topk_ws_elems(g.B, g.total_anchors)), nullptr, NONE},   // keys + the top-k's histograms
        {AT(cand_boxes), WS_F32, DIMS(g.B, L, K, 4), nullptr, "rpn_cand_boxes", 1},
        {AT(cand_scores), WS_F32, DIMS(g.B, L, K), nullptr, "rpn_cand_scores", 1},
        {AT(cand_valid), WS_I32, DIMS(g.B, L, K), nullptr, "rpn_cand_valid", 1},
        {AT(cand_idx), WS_I32, DIMS(g.B, L, K), nullptr, "rpn_cand_idx", 1},
        // One bit per box pair of an item, shared by the RPN NMS (B * 5 items of 1024 candidates) and the detection NMS (B items of
        // P sorted boxes, P * ceil(P / 64) words each): td_engine_create enforces P <= 1024, so B * 1024 * 16 words hold the latter.
        {AT(nms_mask), WS_U64, DIMS(g.B, L, K, K / 64), nullptr, nullptr, NONE},
        {AT(rpn_keep), WS_I32, DIMS(g.B, L, K), nullptr, "rpn_keep", 1},
        {AT(rpn_keep_count), WS_I32, DIMS(g.B, L), nullptr, "rpn_keep_count", 1},
        {AT(props), WS_F32, DIMS(g.B, g.P, 4), nullptr, "proposals", 1},
        {AT(prop_scores), WS_F32, DIMS(g.B, g.P), nullptr, "proposal_scores", 1},
        {AT(prop_count), WS_I32, DIMS(g.B), nullptr, "proposal_count", 1},
        {AT(pooled7), WS_ACT, DIMS(g.B * g.P, 7, 7, g.fpn_c), nullptr, "pooled7", 1},
        {AT(fc1_out), WS_ACT, DIMS(g.B * g.P, g.fc_dim), nullptr, nullptr, NONE},
        {AT(fc2_out), WS_ACT, DIMS(g.B * g.P, g.fc_dim), nullptr, nullptr, NONE},
        {AT(pred_out), WS_F32, DIMS(g.B * g.P, 6), nullptr, "box_pred", 2},
        {AT(dboxes), WS_F32, DIMS(g.B, g.P, 4), nullptr, "det_all_boxes", 3},
        {AT(dscores), WS_F32, DIMS(g.B, g.P), nullptr, "det_all_scores", 3},
        {AT(dflags), WS_I32, DIMS(g.B, g.P), nullptr, "det_flags", 3},
        {AT(sboxes), WS_F32, DIMS(g.B, g.P, 4), nullptr, "det_sorted_boxes", 3},
        {AT(sscores), WS_F32, DIMS(g.B, g.P), nullptr, "det_sorted_scores", 3},
        {AT(sidx), WS_I32, DIMS(g.B, g.P), nullptr, nullptr, NONE},
        {AT(scount), WS_I32, DIMS(g.B), nullptr, "det_sorted_count", 3},
        {AT(det_keep), WS_I32, DIMS(g.B, g.D), nullptr, "det_keep", 3},
        {AT(det_keep_count), WS_I32, DIMS(g.B), nullptr, "det_keep_count", 3},
        {AT(det_boxes_net), WS_F32, DIMS(g.B, g.D, 4), nullptr, "det_boxes_net", 3},
        {AT(pooled14), WS_ACT, DIMS(g.mrows, 14, 14, g.fpn_c), nullptr, "pooled14", 3},
        {AT(mbuf0), WS_ACT, DIMS(g.mrows, 14, 14, g.fpn_c), nullptr, "mask_fcn3", 4},       // the four mask convs alternate between the two:
        {AT(mbuf1), WS_ACT, DIMS(g.mrows, 14, 14, g.fpn_c), nullptr, "mask_fcn4", 4},       // the last two layers' outputs as stored
        {AT(deconv_out), WS_ACT, DIMS(g.mrows, 28, 28, g.deconv_q), nullptr, "mask_deconv", 4},      // pixel-shuffle store (out_mode 1)
        {AT(mask_logits), WS_F32, DIMS(g.mrows, 28, 28), nullptr, "mask_logits", 5},
        {AT(mask_probs_compact), WS_F32, DIMS(g.mrows, 28, 28), nullptr, "mask_probs_compact", 5},
        {AT(total_rows), WS_I32, DIMS(1), ELEMS(4), "mask_total_rows", 4},           // the device row count the mask head's launches read
        {AT(o_boxes), WS_F32, DIMS(g.B, g.D, 4), nullptr, nullptr, NONE},
        {AT(o_scores), WS_F32, DIMS(g.B, g.D), nullptr, nullptr, NONE},
        {AT(o_classes), WS_I32, DIMS(g.B, g.D), nullptr, nullptr, NONE},
        {AT(o_count), WS_I32, DIMS(g.B), nullptr, nullptr, NONE},
        {AT(o_mask_probs), WS_F32, DIMS(g.B, g.D, 28, 28), nullptr, nullptr, NONE},
        {AT(wino_v), WS_F32, DIMS(16, (int64_t)(ws_wino_elems(g) / 16)), nullptr, nullptr, NONE},
        {AT(wino_m), WS_F32, DIMS(16, (int64_t)(ws_wino_elems(g) / 16)), nullptr, nullptr, NONE},
    };
    return rows;
}

size_t ws_row_count(const WsGeom& g) { return ws_rows().size() - (g.wino ? 0 : 2); }
size_t ws_elem_bytes(const WsRow& r, const WsGeom& g) { return r.kind == WS_ACT ? (size_t)g.es : (r.kind == WS_U64 ? 8 : 4); }

size_t ws_alloc_bytes(const WsRow& r, const WsGeom& g, int i) {
    size_t n = 1;
    for (int64_t d : r.dims(g, i).d) n *= d > 0 ? (size_t)d : 1;
    return (r.alloc_elems ? r.alloc_elems(g) : n) * ws_elem_bytes(r, g);
}

// ---- td_workspace_plan (include/treedet.h): the rows above, read out for tests ------------------------------------------------------
extern "C" td_status td_workspace_plan(int precision, int winograd, int post_nms_topk, int detections_per_image, const int32_t* widths, int B,
                                       int Hp, int Wp, td_workspace_row* rows, int cap, int* n_rows) {
    TD_REQUIRE(widths && n_rows && (rows || cap == 0) && cap >= 0, "td_workspace_plan: null argument");
    TD_REQUIRE(precision == TD_PRECISION_FP32 || precision == TD_PRECISION_FP16, "td_workspace_plan: bad precision %d", precision);
    TD_REQUIRE(post_nms_topk >= 1 && post_nms_topk <= 1024 && detections_per_image >= 1 && detections_per_image <= 1024,
               "td_workspace_plan: post_nms_topk / detections_per_image must be in [1,1024]");
    for (int k = 0; k < WS_WIDTHS; ++k) TD_REQUIRE(widths[k] >= 1, "td_workspace_plan: width %d is %d", k, widths[k]);
    TD_REQUIRE(B >= 1 && B <= TD_MAX_BATCH && Hp >= 64 && Wp >= 64 && Hp % 32 == 0 && Wp % 32 == 0, "td_workspace_plan: bad geometry B=%d %dx%d", B, Hp, Wp);
    const WsGeom g = ws_geom(precision, winograd != 0, post_nms_topk, detections_per_image, widths, B, Hp, Wp);
    int n = 0;
    for (size_t k = 0; k < ws_row_count(g); ++k) {
        const WsRow& r = ws_rows()[k];
        for (int i = 0; i < r.count; ++i, ++n) {
            if (n >= cap) continue;
            td_workspace_row& o = rows[n];
            o = td_workspace_row{};
            snprintf(o.name, sizeof o.name, r.count > 1 ? "%s[%d]" : "%s", r.name, i);
            if (r.pub) snprintf(o.public_name, sizeof o.public_name, r.pub, i + 2);
            o.kind = r.kind;
            o.elem_size = (int32_t)ws_elem_bytes(r, g);
            o.phase = r.phase;
            for (int d = 0; d < 4; ++d) o.dims[d] = r.dims(g, i).d[d];
            o.alloc_bytes = (int64_t)ws_alloc_bytes(r, g, i);
        }
    }
    *n_rows = n;
    if (n > cap) {
        td_set_error("td_workspace_plan: %d rows, room for %d", n, cap);
        return TD_ERR_CAPACITY;
    }
    return TD_OK;
}
