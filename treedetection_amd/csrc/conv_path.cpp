// The path rule of the forward's contractions (conv_path.h; exported for tests and tools as td_conv_path, engine.cpp).
#include "conv_path.h"
#include "../../include/treedet.h"

#include <algorithm>

bool wino43_fused_ok(int B, int H, int W, int C, int N) {
    const long long T = (long long)B * ((H + 3) / 4) * ((W + 3) / 4);
    return (C == 128 || C == 256 || C == 512) && N >= 64 && N % 64 == 0 && 36ull * (unsigned long long)T * C * 4 < 0xfffffff0ull - (1u << 20) &&
           36ull * (unsigned long long)N * C * 4 < 0xfffffff0ull - (1u << 20) && (unsigned long long)B * H * W * N * 4 < 0xfffffff0ull - (1u << 20);
}

ConvPath conv_path(const ConvRules& r, const ConvSite& s) {
    const ConvLayerFacts& L = s.L;
    const int Ho = (s.H + 2 * s.pad - L.kh) / s.stride + 1, Wo = (s.W + 2 * s.pad - L.kw) / s.stride + 1;
    const bool fp32 = r.precision == TD_PRECISION_FP32;
    const int maxc = std::max(L.cin, L.cout);
    ConvPath p{};
    p.head = HEAD_OWN_LAUNCH;
    p.slab_tiles = r.wino_slab > 0 ? r.wino_slab : (1 << 30);
    auto key = [&](int k2, long long rows, int flags) {
        p.tune = true;
        p.key[0] = L.cout; p.key[1] = L.cin; p.key[2] = k2; p.key[3] = (int)rows; p.key[4] = flags;
    };
    const bool head1x1 = s.has_head && r.fuse_head && !s.m_dyn && s.relu && L.cout == 256 && s.head.cin == 256 && s.head.kh == 1 && s.head.kw == 1 &&
                         s.head.cout <= 32 && !s.head.scale;
    // Winograd: stride-1 3x3 layers of the fp32 engine whose planes fit the workspace (a device row count: even maps only).
    // Measured on the R50 / R101 layer set (profiles/r02_tile_choices.txt): every 3x3 layer with at least 128 channels on both sides
    // is faster through Winograd at every map size from 13x13 to 200x200 (1.3-1.9x); 64 -> 64 (res2) is HBM-bound on the
    // transforms and stays direct.
    const long long T22 = std::min<long long>((long long)s.B * ((s.H + 1) / 2) * ((s.W + 1) / 2), p.slab_tiles);
    const bool wino = fp32 && r.winograd && L.wino_u && s.stride == 1 && s.pad == 1 && !s.res && s.out_mode == 0 &&
                      (!s.m_dyn || ((s.H | s.W) & 1) == 0) && (size_t)16 * T22 * (size_t)maxc <= r.wino_elems && L.cin >= r.wino_minc &&
                      L.cout >= r.wino_minc;
    if (!wino) {
        // the split rule's layers (the bank exists by td_engine::f32_split; plain output, static rows, no head)
        const bool split = L.w_split && fp32 && s.out_mode == 0 && !s.m_dyn && !s.has_head && s.pad == 0;
        p.form = split ? CONV_SPLIT : CONV_DIRECT;
        key(L.kh * 16 + L.kw, (long long)s.B * Ho * Wo, s.stride * 4 + s.out_mode * 2 + (s.res ? 1 : 0) + (split ? 128 : 0));
        if (head1x1 && !fp32 && s.out_mode == 0 && !s.res && s.head.out_f32) p.head = HEAD_IF_TILE_OWNS_256;
        return p;
    }
    // F(4x4,3x3) on the large maps: 2.25 multiplies per output instead of 4
    const int tiles_img = ((s.H + 3) / 4) * ((s.W + 3) / 4);
    const long long T43 = (long long)s.B * tiles_img;
    const bool f43 = L.wino_u43 && r.wino43_min > 0 && s.H >= r.wino43_min && s.W >= r.wino43_min && (size_t)36 * T43 * (size_t)maxc <= r.wino_elems &&
                     T43 * maxc < (1ll << 31);
    if (!f43) {
        p.form = CONV_WINO22;
        if (!r.wino_fused) key(1 * 16 + 1, T22, 4 + 32);
        return p;
    }
    // The fold (td_engine::wino_fold): per-image map size and channels only. A layer with a 1x1 head — the RPN conv — folds only on
    // the 160 x 160+ maps (bit 32): its head then runs as a launch of its own on the stored map, 1 000 + ~70 us against 1 280 us
    // for the three-launch form with the head in its output transform; on the smaller maps that form wins.
    // (Device-side RoI count: ALL B reserved RoIs are one group, so the 32-bit plane offsets must hold them — about 7 279 RoIs of
    // 14 x 14 x 256; past that the layer keeps the three-launch form. Still a rule on reserved shapes only.)
    const int hw = s.H * s.W, wf = r.wino_fold;
    const bool head = s.has_head, dyn = s.m_dyn;
    const bool fold = wf > 0 && wino43_fused_ok(dyn ? s.B : 1, s.H, s.W, L.cin, L.cout) &&
                      (((wf & 1) && !dyn && (!head || (wf & 32)) && ((L.cin == 256 && hw >= 160 * 160) || (L.cin == 128 && hw >= 80 * 80))) ||
                       ((wf & 2) && dyn && !head) || ((wf & 4) && !dyn && !head && L.cin == 256 && hw >= 80 * 80) ||
                       ((wf & 8) && !dyn && !head && hw >= 40 * 40) || ((wf & 16) && !dyn && !head));
    if (fold) {
        p.form = CONV_WINO43_FOLD;
        const unsigned long long room = 0xfffffff0ull - (2u << 20);
        const unsigned long long gmax = std::min(room / (36ull * tiles_img * (unsigned long long)maxc * 4ull), room / (16ull * tiles_img * L.cout * 4ull));
        p.fold_group = dyn ? s.B : (int)std::max<unsigned long long>(1ull, std::min<unsigned long long>(gmax, s.B));
        return p;
    }
    p.form = CONV_WINO43;
    // the split twin of the F(4x4) bank (td_engine::f32_split_wino): the planes contract on the split-bf16 tiles. Static rows only;
    // the layer and the per-image map decide, never the batch (rows accumulate independently of T)
    p.split_planes = L.w_split && !dyn;
    key(1 * 16 + 1, T43, 4 + 64 + (p.split_planes ? 128 : 0));
    // the head rides in the output transform: bit-identical to the separate launch
    if (head1x1) p.head = HEAD_IN_TRANSFORM;
    return p;
}
