// The engine's workspace plan (workspace.cpp; host only, no HIP calls): every device buffer td_engine_reserve allocates is ONE row of
// ws_rows() — the pointer it fills, its element kind, its extents and allocation size as functions of the geometry, the name and the
// phase under which td_engine_tensor publishes it. td_engine_reserve walks the rows at the reserved geometry, forward_impl publishes
// them at that of the batch in hand, td_workspace_plan (include/treedet.h) reads them out for tests: nobody else states a shape.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// The device pointers the rows fill (td_engine derives from it: the launch code reads e->res[2], e->props, ...)
struct Workspace {
    // activations (element type = engine precision)
    void *stem_out = nullptr, *pool_out = nullptr, *t1[4] = {}, *t2[4] = {}, *scb[4] = {}, *res[4] = {}, *xtmp[4] = {}, *inner[4] = {},
         *pfeat[5] = {}, *rpn_t = nullptr, *pooled7 = nullptr, *fc1_out = nullptr, *fc2_out = nullptr, *pooled14 = nullptr, *mbuf0 = nullptr,
         *mbuf1 = nullptr, *deconv_out = nullptr;
    float *rpn_headbuf[5] = {}, *cand_boxes = nullptr, *cand_scores = nullptr, *props = nullptr, *prop_scores = nullptr, *pred_out = nullptr,
          *dboxes = nullptr, *dscores = nullptr, *sboxes = nullptr, *sscores = nullptr, *det_boxes_net = nullptr, *mask_logits = nullptr,
          *mask_probs_compact = nullptr, *wino_v = nullptr, *wino_m = nullptr, *o_boxes = nullptr, *o_scores = nullptr, *o_mask_probs = nullptr;
    int *cand_valid = nullptr, *cand_idx = nullptr, *rpn_keep = nullptr, *rpn_keep_count = nullptr, *prop_count = nullptr, *dflags = nullptr,
        *sidx = nullptr, *scount = nullptr, *det_keep = nullptr, *det_keep_count = nullptr, *total_rows = nullptr, *o_classes = nullptr,
        *o_count = nullptr;               // (o_*: the outputs' fallback when the caller passes NULL fields)
    uint32_t* key_ws = nullptr; unsigned long long* nms_mask = nullptr;
};

// Everything the shapes depend on
struct WsGeom {
    int B, Hp, Wp, h[5], w[5];        // h x w: the maps of p2 .. p6
    int total_anchors;        // per image, all levels
    int P, D, mrows;          // post_nms_topk, detections_per_image, B * D
    int es;                   // bytes of an activation element (engine precision)
    bool wino;                // fp32 engine with the Winograd switch on: the V / M planes exist
    // the widths the loader found, in the order of ws_geom's list: c1 / c2 / c3 = cout of a stage's first block, deconv_q = deconv.cout / 4
    int stem_c, c1[4], c2[4], c3[4], fpn_c, fc_dim, deconv_q;
};
constexpr int WS_WIDTHS = 16;
WsGeom ws_geom(int precision, bool winograd, int P, int D, const int32_t widths[WS_WIDTHS], int B, int Hp, int Wp);

enum WsKind { WS_ACT, WS_F32, WS_I32, WS_U32, WS_U64 };         // WS_ACT: float32 or float16 by the engine's precision
struct WsDims { int64_t d[4]; };                                // 0-padded, as td_engine_tensor reports them
struct WsRow {
    const char* name;         // the Workspace member, where it lies, and how many pointers it holds (an indexed family: res[4])
    size_t offset; int count;
    WsKind kind;
    WsDims (*dims)(const WsGeom& g, int i);       // i: index within the family
    size_t (*alloc_elems)(const WsGeom& g);       // null: the product of the extents
    const char* pub;          // public name, %d = i + 2 in a family ("res%d": res2 .. res5); null: not published
    int phase;                // the name exists once this phase of the forward has run (6, the stem pre-phase: after it or after phase 0)
};
const std::vector<WsRow>& ws_rows();              // (the two Winograd rows come last and exist only where g.wino: ws_row_count)
size_t ws_row_count(const WsGeom& g);
size_t ws_elem_bytes(const WsRow& r, const WsGeom& g);
size_t ws_alloc_bytes(const WsRow& r, const WsGeom& g, int i);
size_t ws_wino_elems(const WsGeom& g);            // floats in each of wino_v / wino_m (ConvRules::wino_elems); 0 without g.wino
inline void** ws_slot(Workspace* w, const WsRow& r, int i) { return reinterpret_cast<void**>(reinterpret_cast<char*>(w) + r.offset) + i; }
