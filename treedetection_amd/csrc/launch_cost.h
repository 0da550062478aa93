// What one launch of the contraction family costs, for the engine's two books (td_engine_profile_read by category,
// td_engine_profile_classes by speed-of-light class): ONE description per launch family (launch_cost.cpp; host only, no HIP, no
// environment, no engine). The forward (engine.cpp) hands the record to its booking bracket (ProfScope) and does no arithmetic.
#pragma once
#include "conv_path.h"

struct LaunchCost {
    int cat = -1;              // category of td_engine_profile_read; -1: a step of a sequence that is booked as a whole
    int cls = -1;              // TD_CLS_*; -1: a sequence whose steps book their classes
    double exec_flops = 0.0;   // FLOPs the MFMA pipe really executes: the class books and category 8 ("executed")
    double cls_bytes = 0.0;    // class books: the bytes the chosen algorithm moves (V / M planes included)
    double flops = 0.0;        // category books: algorithmic FLOPs (2 M N K of every reference layer in the launch) ...
    double bytes = 0.0;        // ... and bytes: every tensor of every LAYER once, so a fused launch books its unfused twin's
    int layers = 1;            // reference layers the launch stands for: what launches[cat] counts
    bool wino = false;         // a layer on the Winograd path: what launches[8] counts
};
enum { WINO_STEP_INPUT, WINO_STEP_GEMM, WINO_STEP_OUTPUT };      // the steps of a Winograd sequence (wino_run's hook names them)

// A contraction of run_conv: the launch itself (direct, split) or the whole Winograd sequence (cls = -1); head_fused: the 1x1 head
// rides along. A device row count (the mask head) books time only.
LaunchCost conv_cost(int precision, const ConvSite& s, const ConvPath& p, bool head_fused);
// One step of that sequence (cat = -1). n: the tiles of the F(2x2) slab, or the images of the F(4x4) launch (folded: of the group)
LaunchCost wino_step_cost(const ConvSite& s, const ConvPath& p, bool fused_input, bool head_fused, int step, long long n);
// The bottleneck tail on M rows: conv2 (3x3 mid -> mid; split: on split-bf16) + conv3 (1x1 mid -> cout) + shortcut, or (mid_store) conv2 alone
LaunchCost tail_cost(int precision, long long M, int mid, int cout, bool split, bool mid_store);
// The grouped launch of the fp16 engine: one 3x3 layer shape (cin -> 256) on nl pyramid levels; head_cout > 0: with the 1x1 head
LaunchCost grouped_cost(int B, int cin, const int* Hs, const int* Ws, int nl, int head_cout);
