// The crown stage's two box-pair passes (reference TreeDetection/postprocessing.py: filter_polygons_by_iou_and_area 349-406,
// process_containment_features 408-476) without their N x N matrices: the pair tests run here, only the sparse result is stored.
//
// The arithmetic is the host functions' (postprocessing.py: filter_polygons_by_iou_and_area, containment), operation for
// operation, every float operation rounded on its own (-ffp-contract=off, IEEE division):
//   connected(i, j)   iw = max(0, min(x2i, x2j) - max(x1i, x1j)), ih likewise, inter = iw * ih, area = (x2 - x1) * (y2 - y1),
//                     iou = inter / ((area_i + area_j) - inter) in float32, iou > iou_threshold;   AND
//                     d = |a_i - a_j| / max(a_i, a_j) on the float16 areas the way numpy evaluates half arithmetic — both operands
//                     widened to float32, one float32 operation, the result rounded to half, after EACH operation — d < area_threshold
//                     (a half). NaN (0/0, inf - inf, inf/inf) fails every comparison.
//   containment       ratio[i][j] = inter / area_j;  num_contained[i] = #{j != i : ratio[i][j] >= t},
//                     is_contained[i] = any j != i with ratio[j][i] >= t — inter is symmetric, so the owner of row i has both.
// A pair whose boxes do not overlap (iw or ih not positive) is skipped before any of this. That cannot change an answer under the
// callers' preconditions (finite coordinates, finite positive float32 areas, iou_threshold >= 0, containment threshold > 0): inter is
// then +0, iou = 0 / (positive) = 0 is not > a threshold >= 0 and ratio = 0 / (positive) = 0 is not >= a threshold > 0.
//
// Row-owner form: a workgroup of 256 threads owns 256 rows — box, float32 area, float16 area of one crown per thread, in
// registers — and walks one column chunk of PAIR_CHUNK crowns staged once in LDS; every lane reads the same column entry (a
// broadcast: no bank conflicts). Grid = row blocks x column chunks (20 000 crowns: 79 x 20 = 1 580 workgroups); the chunks' partial
// results of a row meet in int32 atomicAdd / atomicOr on outputs the entry points zero on the same stream.
// PAIR_CHUNK = 1024: 1024 x (16 B box + 4 B area + 4 B half area) = 24 576 B of LDS per workgroup, six workgroups (24 waves) per
// CU of 160 KiB.
// Two passes over the same inline pair test (they cannot disagree): count → the caller's exclusive prefix sum → fill (a per-row
// cursor; the order of a row's entries is unspecified).
#include "common.h"

namespace {

constexpr int PAIR_ROWS = 256;
constexpr int PAIR_CHUNK = 1024;
constexpr int PAIR_MAX_N = 65535 * PAIR_CHUNK;     // the column chunks are gridDim.y, which ends at 65 535 (67 107 840 crowns)

struct PairArgs {
    const float* boxes;             // [n][4] x1, y1, x2, y2
    const __half* areas;            // [n] float16 polygon areas (null: containment only)
    int n;
    float iou_thr;
    uint16_t area_thr_bits;         // a float16
    float contain_thr;
    int32_t* counts;                // [n] connected j != i (count pass; null: containment only)
    int32_t* num_contained;         // [n] (count pass; null: no containment)
    int32_t* is_contained;          // [n] 0 / 1
    const int64_t* row_start;       // [n + 1] (fill pass)
    int32_t* cursor;                // [n] zeroed (fill pass)
    int32_t* cols;                  // [row_start[n]] (fill pass)
};

__device__ __forceinline__ float half_round(float v) { return __half2float(__float2half_rn(v)); }

// the intersection of two overlapping boxes; false = disjoint (inter would be +0)
__device__ __forceinline__ bool box_inter(const float4& a, const float4& b, float& inter) {
    const float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x);
    const float ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    if (!(iw > 0.f && ih > 0.f)) return false;
    inter = iw * ih;
    return true;
}

// the de-duplication mask of an overlapping pair
__device__ __forceinline__ bool pair_connected(float inter, float area_i, float area_j, float harea_i, float harea_j, float iou_thr,
                                               float area_thr) {
    const float iou = inter / ((area_i + area_j) - inter);
    if (!(iou > iou_thr)) return false;
    const float diff = fabsf(half_round(harea_i - harea_j));
    const float big = harea_i > harea_j ? harea_i : harea_j;      // (a NaN area has made diff NaN already)
    return half_round(diff / big) < area_thr;
}

template <bool FILL>
__global__ __launch_bounds__(PAIR_ROWS) void crown_pairs_kernel(const PairArgs A) {
    __shared__ float4 s_box[PAIR_CHUNK];
    __shared__ float s_area[PAIR_CHUNK];
    __shared__ float s_harea[PAIR_CHUNK];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * PAIR_ROWS + tid;
    const int j0 = blockIdx.y * PAIR_CHUNK;
    const int nj = min(PAIR_CHUNK, A.n - j0);
    const float4* boxes = reinterpret_cast<const float4*>(A.boxes);
    for (int k = tid; k < nj; k += PAIR_ROWS) {
        const float4 b = boxes[j0 + k];
        s_box[k] = b;
        s_area[k] = (b.z - b.x) * (b.w - b.y);
        s_harea[k] = A.areas ? __half2float(A.areas[j0 + k]) : 0.f;
    }
    __syncthreads();
    if (i >= A.n) return;
    const float4 bi = boxes[i];
    const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
    const float harea_i = A.areas ? __half2float(A.areas[i]) : 0.f;
    const float area_thr = __half2float(__ushort_as_half(A.area_thr_bits));
    const bool filter = FILL || A.counts != nullptr;
    const bool contain = !FILL && A.num_contained != nullptr;
    const int64_t base = FILL ? A.row_start[i] : 0;
    const int64_t end = FILL ? A.row_start[i + 1] : 0;
    int connected = 0, contains = 0, contained = 0;
    for (int k = 0; k < nj; ++k) {
        float inter;
        if (!box_inter(bi, s_box[k], inter) || j0 + k == i) continue;
        const float area_j = s_area[k];
        if (filter && pair_connected(inter, area_i, area_j, harea_i, s_harea[k], A.iou_thr, area_thr)) {
            if (FILL) {
                const int64_t at = base + atomicAdd(&A.cursor[i], 1);
                if (at < end) A.cols[at] = j0 + k;          // (the count pass ran the same test: always inside the row)
            } else {
                ++connected;
            }
        }
        if (contain) {
            contains += inter / area_j >= A.contain_thr;
            contained |= inter / area_i >= A.contain_thr;
        }
    }
    if (FILL) return;
    if (connected) atomicAdd(&A.counts[i], connected);
    if (contains) atomicAdd(&A.num_contained[i], contains);
    if (contained) atomicOr(&A.is_contained[i], 1);
}

dim3 pair_grid(int n) { return dim3(td_cdiv(n, PAIR_ROWS), td_cdiv(n, PAIR_CHUNK)); }

}  // namespace

extern "C" td_status td_crown_pairs_count(const float* boxes, const uint16_t* areas_f16, int n, float iou_threshold,
                                          uint16_t area_threshold_f16, int32_t* counts, float containment_threshold,
                                          int32_t* num_contained, int32_t* is_contained, void* stream) {
    TD_REQUIRE(boxes && (counts || num_contained), "td_crown_pairs_count: null pointer (boxes, and counts or num_contained)");
    TD_REQUIRE(!counts || areas_f16, "td_crown_pairs_count: null pointer (counts without areas_f16)");
    TD_REQUIRE(!num_contained == !is_contained, "td_crown_pairs_count: null pointer (num_contained and is_contained go together)");
    TD_REQUIRE(n >= 1, "td_crown_pairs_count: n = %d, at least one crown is needed", n);
    TD_REQUIRE(n <= PAIR_MAX_N, "td_crown_pairs_count: n = %d, at most %d crowns fit one launch", n, PAIR_MAX_N);
    TD_REQUIRE(aligned16(boxes), "td_crown_pairs_count: boxes must be 16-byte aligned (they are read as float4)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (counts) TD_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n, s));
    if (num_contained) {
        TD_HIP_CHECK(hipMemsetAsync(num_contained, 0, sizeof(int32_t) * (size_t)n, s));
        TD_HIP_CHECK(hipMemsetAsync(is_contained, 0, sizeof(int32_t) * (size_t)n, s));
    }
    PairArgs A{};
    A.boxes = boxes;
    A.areas = reinterpret_cast<const __half*>(areas_f16);
    A.n = n;
    A.iou_thr = iou_threshold;
    A.area_thr_bits = area_threshold_f16;
    A.contain_thr = containment_threshold;
    A.counts = counts;
    A.num_contained = num_contained;
    A.is_contained = is_contained;
    hipLaunchKernelGGL(crown_pairs_kernel<false>, pair_grid(n), dim3(PAIR_ROWS), 0, s, A);
    TD_KERNEL_CHECK();
    return TD_OK;
}

extern "C" td_status td_crown_pairs_fill(const float* boxes, const uint16_t* areas_f16, int n, float iou_threshold,
                                         uint16_t area_threshold_f16, const int64_t* row_start, int32_t* cursor, int32_t* cols,
                                         void* stream) {
    TD_REQUIRE(boxes && areas_f16 && row_start && cursor && cols, "td_crown_pairs_fill: null pointer");
    TD_REQUIRE(n >= 1, "td_crown_pairs_fill: n = %d, at least one crown is needed", n);
    TD_REQUIRE(n <= PAIR_MAX_N, "td_crown_pairs_fill: n = %d, at most %d crowns fit one launch", n, PAIR_MAX_N);
    TD_REQUIRE(aligned16(boxes), "td_crown_pairs_fill: boxes must be 16-byte aligned (they are read as float4)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TD_HIP_CHECK(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n, s));
    PairArgs A{};
    A.boxes = boxes;
    A.areas = reinterpret_cast<const __half*>(areas_f16);
    A.n = n;
    A.iou_thr = iou_threshold;
    A.area_thr_bits = area_threshold_f16;
    A.row_start = row_start;
    A.cursor = cursor;
    A.cols = cols;
    hipLaunchKernelGGL(crown_pairs_kernel<true>, pair_grid(n), dim3(PAIR_ROWS), 0, s, A);
    TD_KERNEL_CHECK();
    return TD_OK;
}
