// GDAL's separable triangle-filter resampler on a raster that lies in HBM, with the crown stage's NDVI rule fused into its
// second pass (postprocessing.py: resample_bilinear_gdal + ndvi_from_rgbi, which stay the description of the values).
//
// The filter taps are NOT computed here: Python flattens postprocessing._decimation_weights per axis into start[n_dst],
// count[n_dst], offset[n_dst] and one float32 weight array (the weights the host path multiplies by) and uploads them. Both
// passes evaluate, per output and per selected band,
//     acc = 0;  for taps in ascending source index:  acc = acc + (float)sample * w        (float32, multiply and add rounded separately)
// which is the host function's arithmetic in a fixed order.
//
//   rows pass     source uint8 [H][W][C] pixel-interleaved (C <= 4) or float32 [H][W]  →  tmp float32 [nb][H][out_w]
//                 One workgroup = 256 neighbouring outputs of RS_ROWS consecutive rows. Neighbouring outputs share most of their
//                 taps (factor 0.2: ten-wide windows five pixels apart), so the workgroup stages the source span its 256 outputs
//                 cover ONCE per row in LDS — one coalesced dword per pixel (the four bands of an RGBI pixel, or one float) — and
//                 every tap is an LDS read; the selected bands are picked out of the dword there. A span that does not fit the
//                 stage (a decimation beyond ~1 / 30) or a pixel that is not one dword (uint8 with C < 4) reads its taps from
//                 global memory instead: same values, same order.
//   columns pass  tmp → dst, lanes along out_w: every tap row is one coalesced read. Output fused, three modes:
//                 f32   planar float32 [nb][out_h][out_w]
//                 u8    clip(floor(v + 0.5), 0, 255), planar uint8 (the host rule for integer rasters)
//                 ndvi  two bands (red, near-infrared) rounded to uint8 as above, then in float64
//                       (nir / 255 - red / 255) / (nir / 255 + red / 255 + 1e-10), rounded once to float32 [out_h][out_w]
//
// The tap tables lie in device memory, so the host cannot look at them: the Python wrapper validates them before the upload,
// and the kernels clamp every entry to the source and to the weight array on top of that — a table that points outside reads
// nothing and contributes nothing instead of faulting. HBM-bound; no matrix work.
#include "common.h"
#include <climits>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_STAGE = 8192;      // dwords of one row's source span held in LDS (32 KiB: five workgroups per CU)
constexpr int RS_ROWS = 4;          // rows per workgroup of the rows pass: the tap table entries are loaded once for all of them

struct AxisTaps {
    const int32_t* start;           // [n_dst] first source index
    const int32_t* count;           // [n_dst] taps
    const int32_t* offset;          // [n_dst] position of the first weight
    const float* weights;           // [n_weights]
    int n_dst;
    long long n_weights;
};

struct RowsArgs {
    const void* src;
    int H, W, C;
    int nb;
    int band[4];
    AxisTaps x;
    float* tmp;                     // [nb][H][out_w]
    int nseg;                       // workgroups along a row
};

struct ColsArgs {
    const float* tmp;               // [nb][H][out_w]
    int H, out_w, nb;
    AxisTaps y;
    void* dst;
    int mode;
    int nseg;
};

// one table entry, clamped to [0, n_src) and to the weight array: (start, count, weights of the entry)
__device__ __forceinline__ void load_taps(const AxisTaps& t, int j, int n_src, int& st, int& cnt, const float*& w) {
    st = t.start[j];
    cnt = t.count[j];
    const long long off = t.offset[j];
    st = st < 0 ? 0 : (st > n_src ? n_src : st);
    cnt = cnt > n_src - st ? n_src - st : cnt;
    if (cnt < 0 || off < 0 || off + cnt > t.n_weights) cnt = 0;
    w = t.weights + (cnt > 0 ? off : 0);
}

template <bool F32>
__global__ __launch_bounds__(RS_THREADS) void resample_rows_kernel(const RowsArgs A) {
    __shared__ uint32_t s_px[RS_STAGE];
    __shared__ int s_lo, s_hi;
    const int tid = threadIdx.x;
    const int seg = (int)(blockIdx.x % (unsigned)A.nseg);
    const int row0 = (int)(blockIdx.x / (unsigned)A.nseg) * RS_ROWS;
    const int row1 = row0 + RS_ROWS < A.H ? row0 + RS_ROWS : A.H;
    const int j = seg * RS_THREADS + tid;
    const int out_w = A.x.n_dst;
    int st = 0, cnt = 0;
    const float* w = nullptr;
    if (j < out_w) load_taps(A.x, j, A.W, st, cnt, w);
    // the source span of this workgroup's outputs
    if (tid == 0) {
        s_lo = INT_MAX;
        s_hi = 0;
    }
    __syncthreads();
    if (cnt > 0) {
        atomicMin(&s_lo, st);
        atomicMax(&s_hi, st + cnt);
    }
    __syncthreads();
    const int lo = s_lo, span = s_hi - lo;
    const bool staged = (F32 || A.C == 4) && span > 0 && span <= RS_STAGE;      // (uniform over the workgroup)
    int shift[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) shift[b] = 8 * A.band[b];
    const uint32_t* src32 = static_cast<const uint32_t*>(A.src);
    const uint8_t* src8 = static_cast<const uint8_t*>(A.src);
    for (int row = row0; row < row1; ++row) {
        const size_t row_px = (size_t)row * A.W;
        if (staged) {
            if (row != row0) __syncthreads();                                   // the previous row's taps have been read
            for (int p = tid; p < span; p += RS_THREADS) s_px[p] = src32[row_px + lo + p];
            __syncthreads();
        }
        if (j >= out_w) continue;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < cnt; ++k) {
            const float wk = w[k];
            if (staged || F32) {
                const uint32_t d = staged ? s_px[st - lo + k] : src32[row_px + st + k];
                if (F32) {
                    acc[0] = __fadd_rn(acc[0], __fmul_rn(__uint_as_float(d), wk));
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (b < A.nb) acc[b] = __fadd_rn(acc[b], __fmul_rn((float)((d >> shift[b]) & 0xffu), wk));
                }
            } else {
                const uint8_t* px = src8 + (row_px + st + k) * A.C;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (b < A.nb) acc[b] = __fadd_rn(acc[b], __fmul_rn((float)px[A.band[b]], wk));
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < A.nb) A.tmp[((size_t)b * A.H + row) * out_w + j] = acc[b];
    }
}

__device__ __forceinline__ float round_u8(float v) {
    float r = floorf(__fadd_rn(v, 0.5f));
    r = r < 0.f ? 0.f : r;
    return r > 255.f ? 255.f : r;
}

__global__ __launch_bounds__(RS_THREADS) void resample_cols_kernel(const ColsArgs A) {
    const int seg = (int)(blockIdx.x % (unsigned)A.nseg);
    const int i = (int)(blockIdx.x / (unsigned)A.nseg);
    const int x = seg * RS_THREADS + (int)threadIdx.x;
    if (x >= A.out_w) return;
    const int out_h = A.y.n_dst;
    int st, cnt;
    const float* w;
    load_taps(A.y, i, A.H, st, cnt, w);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < cnt; ++k) {
        const float wk = w[k];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < A.nb) acc[b] = __fadd_rn(acc[b], __fmul_rn(A.tmp[((size_t)b * A.H + st + k) * A.out_w + x], wk));
    }
    const size_t o = (size_t)i * A.out_w + x, plane = (size_t)out_h * A.out_w;
    if (A.mode == TD_RESAMPLE_F32) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < A.nb) static_cast<float*>(A.dst)[b * plane + o] = acc[b];
    } else if (A.mode == TD_RESAMPLE_U8) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < A.nb) static_cast<uint8_t*>(A.dst)[b * plane + o] = (uint8_t)round_u8(acc[b]);
    } else {
        const double red = (double)round_u8(acc[0]) / 255.0, nir = (double)round_u8(acc[1]) / 255.0;
        static_cast<float*>(A.dst)[o] = (float)((nir - red) / ((nir + red) + 1e-10));
    }
}

bool axis_ok(const int32_t* start, const int32_t* count, const int32_t* offset, const float* weights, int n_dst, long long n_weights) {
    return start && count && offset && weights && n_dst >= 1 && n_weights >= 1;
}

}  // namespace

extern "C" td_status td_resample_gdal_dev(const void* src, int sample_type, int height, int width, int c, const int32_t* bands, int n_bands,
                                          const int32_t* x_start, const int32_t* x_count, const int32_t* x_offset, const float* x_weights,
                                          int out_w, int64_t x_n_weights, const int32_t* y_start, const int32_t* y_count,
                                          const int32_t* y_offset, const float* y_weights, int out_h, int64_t y_n_weights, float* tmp,
                                          void* dst, int mode, void* stream) {
    TD_REQUIRE(src && bands && tmp && dst, "td_resample_gdal_dev: null pointer");
    TD_REQUIRE(sample_type == TD_SAMPLE_U8 || sample_type == TD_SAMPLE_F32, "td_resample_gdal_dev: sample type %d (uint8 = %d, float32 = %d)",
               sample_type, TD_SAMPLE_U8, TD_SAMPLE_F32);
    TD_REQUIRE(mode == TD_RESAMPLE_F32 || mode == TD_RESAMPLE_U8 || mode == TD_RESAMPLE_NDVI, "td_resample_gdal_dev: output mode %d", mode);
    TD_REQUIRE(height >= 1 && width >= 1, "td_resample_gdal_dev: a %d x %d source", height, width);
    TD_REQUIRE(sample_type == TD_SAMPLE_F32 ? c == 1 : (c >= 1 && c <= 4),
               "td_resample_gdal_dev: %d samples per pixel (uint8: 1 .. 4 interleaved, float32: 1)", c);
    TD_REQUIRE(n_bands >= 1 && n_bands <= 4, "td_resample_gdal_dev: %d bands selected (1 .. 4)", n_bands);
    for (int b = 0; b < n_bands; ++b)
        TD_REQUIRE(bands[b] >= 0 && bands[b] < c, "td_resample_gdal_dev: band index %d of a raster with %d bands", bands[b], c);
    TD_REQUIRE(axis_ok(x_start, x_count, x_offset, x_weights, out_w, x_n_weights) && axis_ok(y_start, y_count, y_offset, y_weights, out_h, y_n_weights),
               "td_resample_gdal_dev: tap tables need start / count / offset / weights, n_dst >= 1 and at least one weight (out %d x %d)", out_h, out_w);
    TD_REQUIRE(mode != TD_RESAMPLE_NDVI || n_bands == 2, "td_resample_gdal_dev: mode ndvi takes exactly two bands (red, near-infrared), got %d", n_bands);
    TD_REQUIRE(mode == TD_RESAMPLE_F32 || sample_type == TD_SAMPLE_U8, "td_resample_gdal_dev: modes u8 and ndvi round uint8 samples; the source is float32");
    const int nseg = td_cdiv(out_w, RS_THREADS);
    const long long rows_blocks = (long long)td_cdiv(height, RS_ROWS) * nseg, cols_blocks = (long long)out_h * nseg;
    TD_REQUIRE(rows_blocks <= INT_MAX && cols_blocks <= INT_MAX, "td_resample_gdal_dev: %d x %d -> %d x %d needs more workgroups than one launch holds",
               height, width, out_h, out_w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowsArgs R{};
    R.src = src;
    R.H = height;
    R.W = width;
    R.C = c;
    R.nb = n_bands;
    for (int b = 0; b < 4; ++b) R.band[b] = b < n_bands ? bands[b] : 0;
    R.x = AxisTaps{x_start, x_count, x_offset, x_weights, out_w, (long long)x_n_weights};
    R.tmp = tmp;
    R.nseg = nseg;
    if (sample_type == TD_SAMPLE_F32)
        hipLaunchKernelGGL(resample_rows_kernel<true>, dim3((unsigned)rows_blocks), dim3(RS_THREADS), 0, s, R);
    else
        hipLaunchKernelGGL(resample_rows_kernel<false>, dim3((unsigned)rows_blocks), dim3(RS_THREADS), 0, s, R);
    TD_KERNEL_CHECK();
    ColsArgs V{};
    V.tmp = tmp;
    V.H = height;
    V.out_w = out_w;
    V.nb = n_bands;
    V.y = AxisTaps{y_start, y_count, y_offset, y_weights, out_h, (long long)y_n_weights};
    V.dst = dst;
    V.mode = mode;
    V.nseg = nseg;
    hipLaunchKernelGGL(resample_cols_kernel, dim3((unsigned)cols_blocks), dim3(RS_THREADS), 0, s, V);
    TD_KERNEL_CHECK();
    return TD_OK;
}
