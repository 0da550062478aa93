// The seam strip between two neighbouring rasters, cut on the GPU from the decoded covers of the two windows it touches
// (treedetection_amd/merging.py: merge_images + crop_image without the mosaic). Per SAMPLE of the strip, band-wise as numpy does it:
//   d = fill
//   for each source in order:  if the pixel lies in the rectangle the source may fill  and  equals(d, fill)
//                              and not (the source has its own nodata and equals(s, own)):   d = s
// — rasterio.merge's "first": a value rule on the destination, so a later source shows through where an earlier one holds `fill`.
// equals is merging._equals: exact for integers; float32: isnan(a) for a NaN value, else numpy's isclose(a, python float), which under
// NEP 50 is (|a - (float)v| <= (float)(1e-8 + 1e-5 |v|)  and  isfinite(v))  or  a == (float)v  with the subtraction and both comparisons
// in float32 (one rounding each; -ffp-contract=off, float32 subnormals kept: hipcc's default mode) and the threshold rounded once
// from the double the host computes.
//
// Memory-bound: every source sample of a window is read once, every strip sample written once. A strip row and the source rows
// behind it are runs of consecutive samples, so the kernel works on samples, not pixels: a lane owns one 16-byte unit of the strip
// (16 / sizeof(T) samples, at a 16-byte aligned ADDRESS, whatever the row's length — the first and last unit of a row may be partial
// and are stored sample by sample), a workgroup of 256 lanes a run of 4 KB of one strip row: consecutive lanes, consecutive
// addresses, in a tall narrow strip as in a wide flat one. The unit's source samples are one 16-byte load where the source address
// is 16-byte aligned, four dword loads where it is 4-byte aligned, else loads per sample (a source pitch or origin that moves the
// rows off alignment, a unit that straddles the edge of the rectangle): never a misaligned wide access. Plain stores only.
#include "common.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int SEAM_THREADS = 256;
constexpr int SEAM_UNIT = 16;                       // bytes a lane owns

template <typename T>
struct SeamEq {                                     // equals(a, value) for one value, prepared on the host
    T v;
    float thr;
    int nan, finite;
};

// No branches: with a NaN value e.v is NaN and e.finite is 0, so the first two terms are false and the third is isnan(a); otherwise
// e.nan is 0 and the third is false. Deliberately so, like the select in the kernel: written with `if (e.nan) return ...`, && and || and
// a conditional assignment, the float32 kernel came out of hipcc (ROCm 7.2, -O3) without the assignment on the has_own path — no
// sample of a source with its own nodata was ever copied (tests/test_seam_gpu.py caught it); the integer kernels were right.
template <typename T>
__device__ __forceinline__ int seam_equals(T a, const SeamEq<T>& e) {
    if constexpr (sizeof(T) == 4) {
        return ((int)(fabsf(a - e.v) <= e.thr) & e.finite) | (int)(a == e.v) | (e.nan & (int)(a != a));
    } else {
        return (int)(a == e.v);
    }
}

template <typename T>
struct SeamSrc {
    const T* data;                                  // null: contributes nothing
    int64_t pitch;                                  // SAMPLES per buffer row
    int64_t origin;                                 // sample offset of strip sample (row 0, sample 0) in the buffer: -(row0 * pitch + col0 * spp)
    int r_lo, r_hi;                                 // strip rows it may fill
    int64_t s_lo, s_hi;                             // samples of a strip row it may fill
    int has_own;
    SeamEq<T> own;
};

template <typename T>
struct SeamArgs {
    T* strip;
    int rows;
    int64_t row_samples;                            // cols * spp
    int64_t units;                                  // 16-byte units a row can touch (row_samples / VEC + 2 at most)
    int runs;                                       // workgroups per row
    T fill_value;
    SeamEq<T> fill;
    SeamSrc<T> src[2];
};

template <typename T>
__global__ __launch_bounds__(SEAM_THREADS) void seam_first_kernel(const SeamArgs<T> a) {
    constexpr int VEC = SEAM_UNIT / (int)sizeof(T);
    const int r = blockIdx.x / a.runs;
    const int64_t u = (int64_t)(blockIdx.x % a.runs) * SEAM_THREADS + threadIdx.x;
    if (u >= a.units) return;
    T* row = a.strip + (int64_t)r * a.row_samples;
    // units lie at 16-byte aligned addresses: unit 0 begins `shift` samples before the row does
    const int64_t shift = (int64_t)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) % VEC);
    const int64_t s0 = u * VEC - shift;
    if (s0 >= a.row_samples) return;
    T d[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = a.fill_value;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const SeamSrc<T>& s = a.src[k];
        if (s.data == nullptr || r < s.r_lo || r >= s.r_hi || s0 + VEC <= s.s_lo || s0 >= s.s_hi) continue;
        const T* p = s.data + (s.origin + (int64_t)r * s.pitch + s0);
        T v[VEC];
        const bool whole = s0 >= s.s_lo && s0 + VEC <= s.s_hi;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
        if (whole && addr % 16 == 0) {
            const uint4 w = *reinterpret_cast<const uint4*>(p);
            __builtin_memcpy(v, &w, 16);
        } else if (whole && addr % 4 == 0) {
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const uint32_t*>(p)[q];
            __builtin_memcpy(v, w, 16);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = (s0 + j >= s.s_lo && s0 + j < s.s_hi) ? p[j] : a.fill_value;
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int inside = (int)whole | ((int)(s0 + j >= s.s_lo) & (int)(s0 + j < s.s_hi));
            const int take = inside & seam_equals(d[j], a.fill) & (1 ^ (s.has_own & seam_equals(v[j], s.own)));
            d[j] = take ? v[j] : d[j];
        }
    }
    if (s0 >= 0 && s0 + VEC <= a.row_samples) {
        uint4 w;
        __builtin_memcpy(&w, d, 16);
        *reinterpret_cast<uint4*>(row + s0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (s0 + j >= 0 && s0 + j < a.row_samples) row[s0 + j] = d[j];
    }
}

template <typename T>
SeamEq<T> seam_eq(double value) {
    SeamEq<T> e{};
    if constexpr (sizeof(T) == 4) {
        e.nan = std::isnan(value) ? 1 : 0;
        e.v = (float)value;
        e.thr = (float)(1e-8 + 1e-5 * std::fabs(value));
        e.finite = std::isfinite(value) ? 1 : 0;
    } else {
        e.v = (T)(int64_t)value;
    }
    return e;
}

template <typename T>
td_status seam_first(void* strip, int rows, int cols, int spp, double fill, const td_seam_source* const* sources, hipStream_t s) {
    constexpr int VEC = SEAM_UNIT / (int)sizeof(T);
    if constexpr (sizeof(T) != 4) {
        TD_REQUIRE(fill == std::floor(fill) && fill >= 0 && fill <= (sizeof(T) == 1 ? 255.0 : 65535.0),
                   "td_seam_first_dev: fill %g is not a value of the %d-byte unsigned sample", fill, (int)sizeof(T));
    }
    SeamArgs<T> a{};
    a.strip = static_cast<T*>(strip);
    a.rows = rows;
    a.row_samples = (int64_t)cols * spp;
    a.units = a.row_samples / VEC + 2;
    a.runs = (int)((a.units + SEAM_THREADS - 1) / SEAM_THREADS);
    a.fill = seam_eq<T>(fill);
    a.fill_value = a.fill.v;
    for (int k = 0; k < 2; ++k) {
        const td_seam_source* src = sources[k];
        SeamSrc<T>& d = a.src[k];
        if (src == nullptr || src->data == nullptr) continue;
        TD_REQUIRE(reinterpret_cast<uintptr_t>(src->data) % sizeof(T) == 0, "td_seam_first_dev: source %d is not aligned to its %d-byte samples", k,
                   (int)sizeof(T));
        TD_REQUIRE(src->rows >= 1 && src->pitch >= 1 && src->pitch <= INT32_MAX, "td_seam_first_dev: source %d: %d rows of %lld pixels", k, src->rows,
                   (long long)src->pitch);
        TD_REQUIRE(src->r_lo >= 0 && src->r_lo <= src->r_hi && src->r_hi <= rows && src->c_lo >= 0 && src->c_lo <= src->c_hi && src->c_hi <= cols,
                   "td_seam_first_dev: source %d: rectangle rows %d..%d, columns %d..%d leaves the %d x %d strip", k, src->r_lo, src->r_hi, src->c_lo,
                   src->c_hi, rows, cols);
        if (src->r_lo == src->r_hi || src->c_lo == src->c_hi) continue;         // an empty rectangle fills nothing
        TD_REQUIRE((int64_t)src->r_lo - src->row0 >= 0 && (int64_t)src->r_hi - src->row0 <= src->rows && (int64_t)src->c_lo - src->col0 >= 0 &&
                       (int64_t)src->c_hi - src->col0 <= src->pitch,
                   "td_seam_first_dev: source %d: its rectangle reaches outside its %d x %lld pixels at strip (%d, %d)", k, src->rows,
                   (long long)src->pitch, src->row0, src->col0);
        if constexpr (sizeof(T) != 4) {
            TD_REQUIRE(!src->has_own || (src->own == std::floor(src->own) && src->own >= 0 && src->own <= (sizeof(T) == 1 ? 255.0 : 65535.0)),
                       "td_seam_first_dev: source %d: own nodata %g is not a value of the %d-byte unsigned sample", k, src->own, (int)sizeof(T));
        }
        d.data = static_cast<const T*>(src->data);
        d.pitch = src->pitch * spp;
        d.origin = -((int64_t)src->row0 * d.pitch + (int64_t)src->col0 * spp);
        d.r_lo = src->r_lo;
        d.r_hi = src->r_hi;
        d.s_lo = (int64_t)src->c_lo * spp;
        d.s_hi = (int64_t)src->c_hi * spp;
        d.has_own = src->has_own ? 1 : 0;
        d.own = seam_eq<T>(src->has_own ? src->own : 0.0);
    }
    TD_REQUIRE((int64_t)rows * a.runs <= INT32_MAX, "td_seam_first_dev: a %d x %d strip needs too many workgroups", rows, cols);
    hipLaunchKernelGGL((seam_first_kernel<T>), dim3((unsigned)(rows * a.runs)), dim3(SEAM_THREADS), 0, s, a);
    TD_KERNEL_CHECK();
    return TD_OK;
}

}  // namespace

extern "C" td_status td_seam_first_dev(void* strip, int rows, int cols, int spp, int sample_type, double fill, const td_seam_source* first,
                                       const td_seam_source* second, void* stream) {
    TD_REQUIRE(strip != nullptr, "td_seam_first_dev: null strip");
    TD_REQUIRE(rows >= 1 && cols >= 1 && spp >= 1 && spp <= 4, "td_seam_first_dev: a %d x %d strip of %d samples per pixel", rows, cols, spp);
    TD_REQUIRE(sample_type == TD_SAMPLE_U8 || sample_type == TD_SAMPLE_U16 || sample_type == TD_SAMPLE_F32, "td_seam_first_dev: sample type %d",
               sample_type);
    const int item = sample_type == TD_SAMPLE_U8 ? 1 : sample_type == TD_SAMPLE_U16 ? 2 : 4;
    TD_REQUIRE(reinterpret_cast<uintptr_t>(strip) % item == 0, "td_seam_first_dev: the strip is not aligned to its %d-byte samples", item);
    const td_seam_source* sources[2] = {first, second};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sample_type == TD_SAMPLE_U8) return seam_first<uint8_t>(strip, rows, cols, spp, fill, sources, s);
    if (sample_type == TD_SAMPLE_U16) return seam_first<uint16_t>(strip, rows, cols, spp, fill, sources, s);
    return seam_first<float>(strip, rows, cols, spp, fill, sources, s);
}
