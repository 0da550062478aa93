// The Winograd launch sequences of a stride-1 3x3 layer (fp32), each written once over the launch entries of common.h: the engine
// (engine.cpp run_conv) and the op-level test entry (api.cpp wino_api) both run a layer through wino_run.
#include "common.h"

#include <algorithm>

// The 16 plane contractions of F(2x2,3x3) slab [t0, t0 + n): V [16][n][cin] x U [16][cout][cin] -> M as ONE batched launch, or
// (fused_input) the contraction that reads the layer input x [B,H,W,cin] and transforms it in its A staging
ConvArgs wino_plane_args(const WinoRun& r, int n, long long t0) {
    ConvArgs a{};
    a.w = r.U; a.y = r.M;
    a.Cin = r.cin; a.Cout = r.cout; a.KH = a.KW = 1; a.stride = 1; a.pad = 0;
    a.M = n; a.m_dyn = r.m_dyn; a.m_mul = r.m_dyn ? r.m_mul / 4 : 1;    // even H, W with a device row count: tiles = rows / 4
    a.m_off = (int)t0;
    a.w_bs = (long long)r.cout * r.cin; a.y_bs = (long long)n * r.cout;
    a.tile_cfg = r.gemm_cfg;
    if (r.fused_input) { a.x = r.x; a.B = r.B; a.H = r.H; a.W = r.W; }
    else { a.x = r.V; a.B = 1; a.H = 1; a.W = n; a.Ho = 1; a.Wo = n; a.batch_count = 16; a.x_bs = (long long)n * r.cin; }
    return a;
}

// The 36 plane contractions of F(4x4,3x3) over a whole layer as ONE batched launch: V [36][T][cin] x U -> M [36][T][cout]
// (m_dyn: the planes keep the stride of the full batch, only the live tiles are computed). With the split twin of U (WinoRun::U_split,
// static rows) the same launch runs conv_split_kernel's batched form: w_split and the bank's byte stride ride along, and
// conv_tile_refusal then lets the TILE_SPLIT ids run it and nothing else.
ConvArgs wino43_plane_args(const WinoRun& r) {
    const int tiles_img = ((r.H + 3) / 4) * ((r.W + 3) / 4);
    const long long T = (long long)r.B * tiles_img;
    ConvArgs a{};
    a.x = r.V; a.w = r.U; a.y = r.M;
    a.Cin = r.cin; a.Cout = r.cout; a.KH = a.KW = 1; a.stride = 1; a.pad = 0;
    a.B = 1; a.H = 1; a.W = (int)T; a.Ho = 1; a.Wo = (int)T;
    a.M = (int)T; a.m_dyn = r.m_dyn; a.m_mul = r.m_dyn ? tiles_img : 1;
    a.batch_count = 36; a.x_bs = T * r.cin; a.w_bs = (long long)r.cout * r.cin; a.y_bs = T * r.cout;
    a.tile_cfg = r.gemm_cfg;
    // the split twin (static rows only): the planes contract on the split-bf16 tiles, whose bank stride counts bytes
    if (r.U_split && !r.m_dyn) { a.w_split = r.U_split; a.w_bs = (long long)conv_split_bank_bytes(r.cout, r.cin); }
    return a;
}

td_status wino_run(const WinoRun& r, hipStream_t s, const WinoHook* hook) {
    // one launch, between the caller's books of it (null when nobody keeps any)
#define TD_WINO_STEP(which, n, launch)                  \
    do {                                                \
        if (hook) hook->begin(hook->ctx, which, n);     \
        const td_status st_ = (launch);                 \
        if (hook) hook->end(hook->ctx);                 \
        if (st_ < 0) return st_;                        \
    } while (0)
    if (r.form == CONV_WINO22) {
        // input transform -> ONE batched launch of the 16 plane contractions -> output transform with the layer's scale / bias /
        // ReLU (winograd.hip), slab by slab: V + M of a slab can stay in the Infinity Cache
        const long long T = (long long)r.B * ((r.H + 1) / 2) * ((r.W + 1) / 2);
        for (long long t0 = 0; t0 < T; t0 += r.slab_tiles) {
            const int n = (int)std::min<long long>(r.slab_tiles, T - t0);
            if (!r.fused_input) TD_WINO_STEP(WINO_STEP_INPUT, n, wino_input_launch(r.x, r.B, r.H, r.W, r.cin, r.V, r.m_dyn, r.m_mul, t0, n, s));
            const ConvArgs a = wino_plane_args(r, n, t0);
            TD_WINO_STEP(WINO_STEP_GEMM, n, r.fused_input ? wino_gemm_launch(a, s) : conv2d_launch(a, TD_PRECISION_FP32, s));
            TD_WINO_STEP(WINO_STEP_OUTPUT, n, wino_output_launch(r.M, r.B, r.H, r.W, r.cout, r.scale, r.bias, r.relu, r.y, r.m_dyn, r.m_mul, t0, n, s));
        }
        return TD_OK;
    }
    if (r.form == CONV_WINO43_FOLD) {
        // contraction + output transform in one launch: V and U in, y out (wino_fused.hip), image group by image group
        for (int b0 = 0; b0 < r.B; b0 += r.fold_group) {
            const int Bg = std::min(r.fold_group, r.B - b0);
            const float* xg = r.x + (size_t)b0 * r.H * r.W * r.cin;
            float* yg = r.y + (size_t)b0 * r.H * r.W * r.cout;
            TD_WINO_STEP(WINO_STEP_INPUT, Bg, wino43_input_launch(xg, Bg, r.H, r.W, r.cin, r.V, r.m_dyn, s));
            TD_WINO_STEP(WINO_STEP_GEMM, Bg, wino43_fused_launch(r.V, r.U, Bg, r.H, r.W, r.cin, r.cout, r.scale, r.bias, r.relu, yg, r.m_dyn, s));
        }
        return TD_OK;
    }
    // F(4x4,3x3) of a whole layer: x -> V [36][T][cin] -> 36 batched plane contractions -> M -> y, or (head_w) the 1x1 head
    // contracted inside the output transform (wino43_output_head_kernel): y is not written
    TD_WINO_STEP(WINO_STEP_INPUT, r.B, wino43_input_launch(r.x, r.B, r.H, r.W, r.cin, r.V, r.m_dyn, s));
    TD_WINO_STEP(WINO_STEP_GEMM, r.B, conv2d_launch(wino43_plane_args(r), TD_PRECISION_FP32, s));
    TD_WINO_STEP(WINO_STEP_OUTPUT, r.B, r.head_w ? wino43_output_head_launch(r.M, r.B, r.H, r.W, r.cout, r.scale, r.bias, r.relu, r.head_w, r.head_b, r.head_y, r.head_n, s)
                                                  : wino43_output_launch(r.M, r.B, r.H, r.W, r.cout, r.scale, r.bias, r.relu, r.y, r.m_dyn, s));
    return TD_OK;
#undef TD_WINO_STEP
}
