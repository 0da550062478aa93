// The cost of every launch family of the forward's contractions (launch_cost.h).
#include "launch_cost.h"
#include "../../include/treedet.h"

namespace {
// A split-bf16 contraction: six bf16 MFMAs (192 pipe cycles) per 16 k against 512 for the fp32 MFMAs — its FLOPs enter the executed
// books as its pipe time in units of the fp32 rate; its filters cross HBM as three bf16 pieces per weight.
constexpr double SPLIT_PIPE_FACTOR = 6.0 / 16.0, SPLIT_WEIGHT_BYTES = 6.0;
// The Winograd plane model: P = 16 (F(2x2)) or 36 (F(4x4)) plane products of [T x cin] x [cin x cout]; V / M are P T rows (F(2x2):
// 4x the input / output, F(4x4): 2.25x the padded ones), each crossing HBM once per direction; U is the transformed bank.
struct Planes { double vb, mb, ub, flops; };
Planes planes(bool f22, double T, double cin, double cout, bool split) {
    const double P = f22 ? 16.0 : 36.0;
    return {4.0 * P * T * cin, 4.0 * P * T * cout, (split ? SPLIT_WEIGHT_BYTES : 4.0) * P * cout * cin, 2.0 * P * T * cin * cout * (split ? SPLIT_PIPE_FACTOR : 1.0)};
}
double tiles43(const ConvSite& s) { return (double)s.B * ((s.H + 3) / 4) * ((s.W + 3) / 4); }
double elem_bytes(int precision) { return precision == TD_PRECISION_FP16 ? 2.0 : 4.0; }
}  // namespace

LaunchCost conv_cost(int precision, const ConvSite& s, const ConvPath& p, bool head_fused) {
    const ConvLayerFacts& L = s.L;
    const bool split = p.form == CONV_SPLIT, wino = p.form >= CONV_WINO22;
    const int cls = wino ? -1 : s.m_dyn ? TD_CLS_MASK_HEAD : s.H == 1 && s.W == 1 ? TD_CLS_FC : L.kh == 1 && L.kw == 1 ? TD_CLS_CONV1X1 : TD_CLS_CONV3X3;
    if (s.m_dyn) return {7, cls};
    const int Ho = (s.H + 2 * s.pad - L.kh) / s.stride + 1, Wo = (s.W + 2 * s.pad - L.kw) / s.stride + 1;
    const double M = (double)s.B * Ho * Wo, K = (double)L.kh * L.kw * L.cin, es = elem_bytes(precision), flops = 2.0 * M * L.cout * K;
    const double bytes = es * ((double)s.B * s.H * s.W * L.cin / (s.stride * s.stride) + M * L.cout * (s.res ? 2.0 : 1.0)) + (split ? SPLIT_WEIGHT_BYTES : es) * L.cout * K;
    // F(4x4): the plane products of the padded map; F(2x2): 4 multiplies per output instead of 9 (the map's own size, odd sides too)
    const double pipe = p.form >= CONV_WINO43 ? planes(false, tiles43(s), L.cin, L.cout, p.split_planes).flops : wino ? flops * 4.0 / 9.0 : split ? flops * SPLIT_PIPE_FACTOR : flops;
    if (!head_fused) return {0, cls, pipe, bytes, flops, bytes, 1, wino};
    // the head's FLOPs / bytes join the launch's; its input read and this layer's output write move nothing but stay in the category books
    const double hflops = 2.0 * M * s.head.cout * L.cout, hbytes = 4.0 * M * s.head.cout + es * s.head.cout * L.cout, yb = es * M * L.cout;
    return {0, cls, pipe + hflops, bytes - yb + hbytes, flops + hflops, bytes + (hbytes + yb), 2, wino};
}

LaunchCost wino_step_cost(const ConvSite& s, const ConvPath& p, bool fused_input, bool head_fused, int step, long long n) {
    if (s.m_dyn) return {-1, TD_CLS_MASK_HEAD};
    const ConvLayerFacts& L = s.L;
    const bool f22 = p.form == CONV_WINO22;
    const Planes q = planes(f22, f22 ? (double)n : tiles43(s), L.cin, L.cout, p.split_planes);
    const double share = f22 ? 1.0 : (double)n / s.B;           // folded F(4x4): the image group's part
    const double px = (double)s.B * s.H * s.W, xb = 4.0 * px * L.cin, yb = 4.0 * px * L.cout;
    if (step == WINO_STEP_INPUT) return {-1, TD_CLS_WINO_XFORM, 0.0, (xb + q.vb) * share};
    // (folded: V and U in, y out; F(2x2) with the input transform inside: x in place of V)
    if (step == WINO_STEP_GEMM)
        return {-1, TD_CLS_WINO_GEMM, q.flops * share, p.form == CONV_WINO43_FOLD ? (q.vb + yb) * share + q.ub : (f22 && fused_input ? xb : q.vb) + q.ub + q.mb};
    if (head_fused) return {-1, TD_CLS_WINO_XFORM, 2.0 * px * s.head.cout * L.cout, q.mb + (4.0 * px * s.head.cout + 4.0 * s.head.cout * L.cout)};
    return {-1, TD_CLS_WINO_XFORM, 0.0, q.mb + yb};
}

LaunchCost tail_cost(int precision, long long M_, int mid_, int cout_, bool split, bool mid_store) {
    const double M = (double)M_, mid = mid_, co = cout_, es = elem_bytes(precision), t2b = es * 2.0 * M * mid;
    const double f2 = 2.0 * M * mid * (9.0 * mid), f2pipe = split ? f2 * SPLIT_PIPE_FACTOR : f2, w2b = (split ? SPLIT_WEIGHT_BYTES : es) * 9.0 * mid * mid;
    if (mid_store) return {0, TD_CLS_CONV3X3, f2pipe, t2b + w2b, f2, t2b + w2b};          // t1 in, t2 out, conv2's bank
    const double f3 = 2.0 * M * co * mid, bytes = es * (M * mid + 2.0 * M * co + co * mid) + w2b;      // t1 in, shortcut in, y out, both banks
    return {0, TD_CLS_TAIL, f2pipe + f3, bytes, f2 + f3, bytes + t2b, 2};       // (category: + t2 written and read back by the unfused pair)
}

LaunchCost grouped_cost(int B, int cin, const int* Hs, const int* Ws, int nl, int head_cout) {
    LaunchCost c{0, TD_CLS_CONV3X3};
    c.layers = nl * (head_cout ? 2 : 1);
    for (int l = 0; l < nl; ++l) {
        const double M = (double)B * Hs[l] * Ws[l], K = 9.0 * cin;
        c.flops += 2.0 * M * 256 * K + (head_cout ? 2.0 * M * head_cout * 256 : 0.0);
        c.cls_bytes += 2.0 * (M * cin + (head_cout ? 0.0 : M * 256) + 256 * K) + (head_cout ? 4.0 * M * head_cout + 2.0 * head_cout * 256 : 0.0);
        c.bytes += head_cout ? 2.0 * 2.0 * M * 256 : 0.0;        // the 256-channel map written and read back by a separate head
    }
    c.bytes += c.cls_bytes;
    c.exec_flops = c.flops;
    return c;
}
