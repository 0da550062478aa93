// Treetops in a height raster (td_treetops_dev, treetops.hip; td_treetops, treetops_host.cpp): THE RULE, stated once for both.
//
// Smoothing: two 1-D passes of the caller's symmetric weight table w [2r + 1], axis 0 (along the rows' index) first, then axis 1,
// each output rounded to float32 once. An index outside [0, n) is reflected about the edge (d c b a | a b c d | d c b a) for any
// n, n < r included. One output, in float64, multiply and add rounded separately (no fused multiply-add: -ffp-contract=off):
//     t = in[l] * w[r];   for ii = -r .. -1:  t = t + (in[l + ii] + in[l - ii]) * w[r + ii];   out[l] = (float)t
// — scipy.ndimage.correlate1d's order for a symmetric kernel, so the result is gaussian_filter's (float32 in and out) bit for bit
// when w is the table scipy builds. r = 0 with w = [1.0] leaves the raster as it is.
// Treetop: with s the smoothed raster, pixel (row, col) is a treetop iff s > floor and s >= s' for every non-NaN s' among the
// in-range pixels of the k x k window centred on it (k odd, h = k / 2). A NaN s is never a treetop. Every pixel of a plateau that
// equals its window maximum is a treetop. The window maximum is taken with fmax_nan (a NaN operand is passed over) in any order:
// a maximum is exact. A NaN is a NaN: which NaN a sum of infinities gives (its sign, its payload) is not part of the rule.
// Compiled by hipcc for the device and by g++ for the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TD_TT_HD __host__ __device__ inline
#else
#define TD_TT_HD inline
#endif

namespace tdtops {

// scipy's `reflect` for any i and n >= 1 (64-bit: n may be 2^31 - 1, and i a tile's halo beyond it)
TD_TT_HD int reflect(long long i, int n) {
    if (i >= 0 && i < n) return (int)i;
    const long long p = 2ll * n;
    i %= p;
    if (i < 0) i += p;
    return (int)(i >= n ? p - 1 - i : i);
}

// one output of one pass; at(ii) = the float32 input at l + ii, -r <= ii <= r, already reflected
template <class At>
TD_TT_HD float smooth_one(const double* w, int r, At at) {
    double t = (double)at(0) * w[r];
    for (int ii = -r; ii < 0; ++ii) {
        const double pair = (double)at(ii) + (double)at(-ii);
        const double prod = pair * w[r + ii];
        t = t + prod;
    }
    return (float)t;
}

// the maximum that passes a NaN over: NaN only when both are
TD_TT_HD float fmax_nan(float a, float b) { return b != b ? a : (a != a ? b : (a > b ? a : b)); }

// s against the window maximum m (fmax_nan over the window, s itself included) and the floor
TD_TT_HD bool is_top(float s, float m, float floor) { return s > floor && s >= m; }

TD_TT_HD bool finite64(double v) { return v - v == 0.0; }

// why the call is refused, or nullptr: what both entry points check before anything runs (the pointers are theirs to check)
inline const char* refusal(int rows, int cols, const double* w, int r, int window, float floor) {
    if (rows < 1 || cols < 1 || (int64_t)rows * cols > (int64_t)INT32_MAX) return "rows and cols at least 1 and fewer than 2^31 pixels";
    if (window < 1 || window % 2 == 0) return "the window must be odd and at least 1";
    if (r < 0 || r > (1 << 20)) return "the radius must be between 0 and 2^20";
    if (floor != floor) return "the floor is NaN";
    for (int i = 0; i <= 2 * r; ++i)
        if (!finite64(w[i])) return "a weight is not finite";
    for (int i = 0; i < r; ++i)
        if (w[i] != w[2 * r - i]) return "the weight table is not symmetric";
    return nullptr;
}

}  // namespace tdtops
