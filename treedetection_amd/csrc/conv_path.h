// Which form a convolution layer takes in the forward: ONE pure function over plain data (conv_path.cpp; host only, no HIP, no
// environment, no clock). The forms differ in rounding, so the choice is a fixed rule on the layer's own shape — never the batch
// and never a timing: a batch of 8 equals eight batches of 1 bit for bit, and results do not vary between processes. The engine
// (engine.cpp run_conv) asks it for every contraction; td_conv_path (include/treedet.h) exports it for tests and tools.
#pragma once
#include <cstddef>

// The knobs td_engine_create reads, and the Winograd workspace td_engine_reserve sized
struct ConvRules {
    int precision;        // TD_PRECISION_*
    bool winograd;        // TD_WINOGRAD
    bool wino_fused;      // TD_WINO_FUSED: F(2x2) transforms its input inside the contraction (then nothing of it is tuned)
    int wino_minc;        // fewest channels (both sides) of a 3x3 layer on the Winograd path
    int wino43_min;       // maps at least this large on both sides take F(4x4,3x3); 0 = never
    int wino_fold;        // bit mask of the F(4x4) layers that fold (td_engine::wino_fold)
    int wino_slab;        // tiles per F(2x2) slab; 0 = the whole layer
    bool fuse_head;       // TD_FUSE_HEAD
    size_t wino_elems;    // floats in each of the two workspace planes (V, M)
};
struct ConvLayerFacts {
    int cout, cin, kh, kw;
    bool scale, out_f32;
    bool wino_u, wino_u43, w_split;     // which filter banks the layer has beside its own (w_split of a 3x3 layer: the split twin of its F(4x4) bank)
};
struct ConvSite {
    ConvLayerFacts L;
    int B, H, W, stride, pad;
    bool relu, res;
    int out_mode;
    bool m_dyn;           // the row count lives on the device (the mask head: B = the reserved RoIs)
    int m_mul;
    bool has_head;        // a 1x1 layer that is this layer's only consumer (the RPN's 15-row head)
    ConvLayerFacts head;
};

enum ConvForm { CONV_DIRECT, CONV_SPLIT, CONV_WINO22, CONV_WINO43, CONV_WINO43_FOLD };
// Where the 1x1 head goes. HEAD_IF_TILE_OWNS_256: inside the direct launch when the tuned tile owns all 256 output channels
// (conv_head_capable) — bit-identical to the separate launch either way, so here, and only here, a timing may take part.
enum ConvHead { HEAD_OWN_LAUNCH, HEAD_IN_TRANSFORM, HEAD_IF_TILE_OWNS_256 };

struct ConvPath {
    ConvForm form;
    ConvHead head;
    // The launch shape whose block tile is measured: (cout, cin, kh*16+kw, rows, stride*4 + out_mode*2 + has_residual + flag). Flags:
    // 32 = the 16 batched F(2x2) plane contractions (rows = tiles of a slab), 64 = the 36 of F(4x4) (rows = tiles), 128 = a split
    // layer (tune-cache lines written for its fp32 tiles do not apply). tune = false: the form has no tile to measure.
    bool tune;
    int key[5];
    int slab_tiles;       // F(2x2): tiles per slab
    // folded F(4x4): images per launch pair. The kernel's 32-bit plane offsets hold 4 GB of V: a larger batch runs in image groups,
    // so the layer takes the SAME form at every batch size. (Device-side RoI count: all B reserved RoIs are one group.)
    int fold_group;
    // CONV_WINO43 only: the 36 plane contractions run on the split-bf16 tiles (the layer has the split twin of its F(4x4) bank —
    // ConvLayerFacts::w_split of a 3x3 layer — and static rows); the key then carries flag 128 on top of 64. Not the folded form.
    bool split_planes;
};

ConvPath conv_path(const ConvRules& r, const ConvSite& s);

// shapes wino43_fused_kernel runs (wino_fused.hip): C = 128, 256 or 512, N a multiple of its 64-channel blocks, every tensor it
// addresses with 32-bit offsets below 4 GB
bool wino43_fused_ok(int B, int H, int W, int C, int N);
