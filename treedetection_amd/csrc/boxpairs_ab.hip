// Candidate pairs between TWO box sets (evaluation.py: predictions against annotations) without the n_a x n_b matrix: the pair
// test runs here, only the sparse result is stored. crownpairs.hip pairs a set with itself in float32; this one takes float64
// boxes as they are, so nothing is rounded and no layer is too wide for it.
//
// The rule (include/treedet.h states it): (i, j) is a pair iff every upper coordinate exceeds every lower one on both axes —
//   x2_i > x1_i, x2_j > x1_j, x2_i > x1_j, x2_j > x1_i, and the same in y
// which is min(x2_i, x2_j) > max(x1_i, x1_j) written as comparisons: a NaN fails them all, touching boxes and boxes of zero width
// or height pair with nothing. The first two comparisons of an axis concern one box alone: a row that fails them walks no
// columns, and a column that fails them is staged as four NaNs, so the inner loop is the four cross comparisons.
//
// Row-owner form (crownpairs.hip): a workgroup of 256 threads owns 256 rows of A, one box per thread in registers (8 VGPRs), and
// walks one chunk of AB_CHUNK = 1024 boxes of B staged once in LDS — 1024 x 32 B = 32 768 B per workgroup, five workgroups (20
// waves) per CU of 160 KiB; every lane reads the same column entry (a broadcast: no bank conflicts). Grid = row blocks x column
// chunks; the chunks' partial counts of a row meet in an int32 atomicAdd on an output the entry point zeroes on the same stream.
// Two passes over the same inline test (they cannot disagree): count → the caller's exclusive prefix sum → fill (a per-row
// cursor; the order of a row's entries is unspecified).
#include "common.h"

namespace {

constexpr int AB_ROWS = 256;
constexpr int AB_CHUNK = 1024;
constexpr int AB_MAX_N = 65535 * AB_CHUNK;       // the column chunks are gridDim.y, which ends at 65 535; the rows take the same limit

struct AbArgs {
    const double2* boxes_a;         // [n_a][2] (x1, y1), (x2, y2)
    const double2* boxes_b;         // [n_b][2]
    int n_a, n_b;
    int32_t* counts;                // [n_a] (count pass)
    const int64_t* row_start;       // [n_a + 1] (fill pass)
    int32_t* cursor;                // [n_a] zeroed (fill pass)
    int32_t* cols;                  // [row_start[n_a]] (fill pass)
};

__device__ __forceinline__ bool box_has_area(const double2& lo, const double2& hi) { return hi.x > lo.x && hi.y > lo.y; }

template <bool FILL>
__global__ __launch_bounds__(AB_ROWS) void box_pairs_ab_kernel(const AbArgs A) {
    __shared__ double2 s_lo[AB_CHUNK];
    __shared__ double2 s_hi[AB_CHUNK];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * AB_ROWS + tid;
    const int j0 = blockIdx.y * AB_CHUNK;
    const int nj = min(AB_CHUNK, A.n_b - j0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = tid; k < nj; k += AB_ROWS) {
        double2 lo = A.boxes_b[2 * (size_t)(j0 + k)], hi = A.boxes_b[2 * (size_t)(j0 + k) + 1];
        if (!box_has_area(lo, hi)) lo = hi = make_double2(nan, nan);
        s_lo[k] = lo;
        s_hi[k] = hi;
    }
    __syncthreads();
    if (i >= A.n_a) return;
    const double2 lo = A.boxes_a[2 * (size_t)i], hi = A.boxes_a[2 * (size_t)i + 1];
    if (!box_has_area(lo, hi)) return;
    const int64_t base = FILL ? A.row_start[i] : 0;
    const int64_t end = FILL ? A.row_start[i + 1] : 0;
    int found = 0;
    for (int k = 0; k < nj; ++k) {
        const double2 cl = s_lo[k], ch = s_hi[k];
        if (!(hi.x > cl.x && ch.x > lo.x && hi.y > cl.y && ch.y > lo.y)) continue;
        if (FILL) {
            const int64_t at = base + atomicAdd(&A.cursor[i], 1);
            if (at < end) A.cols[at] = j0 + k;          // (the count pass ran the same test: always inside the row)
        } else {
            ++found;
        }
    }
    if (!FILL && found) atomicAdd(&A.counts[i], found);
}

td_status check_sets(const char* who, const double* boxes_a, int n_a, const double* boxes_b, int n_b) {
    TD_REQUIRE(n_a >= 1 && n_b >= 1, "%s: n_a = %d, n_b = %d, at least one box is needed on either side", who, n_a, n_b);
    TD_REQUIRE(n_a <= AB_MAX_N && n_b <= AB_MAX_N, "%s: n_a = %d, n_b = %d, at most %d boxes on either side fit one launch", who, n_a, n_b,
               AB_MAX_N);
    TD_REQUIRE(aligned16(boxes_a) && aligned16(boxes_b), "%s: the boxes must be 16-byte aligned (they are read as double2)", who);
    return TD_OK;
}

dim3 ab_grid(int n_a, int n_b) { return dim3(td_cdiv(n_a, AB_ROWS), td_cdiv(n_b, AB_CHUNK)); }

}  // namespace

extern "C" td_status td_box_pairs_ab_count(const double* boxes_a, int n_a, const double* boxes_b, int n_b, int32_t* counts, void* stream) {
    TD_REQUIRE(boxes_a && boxes_b && counts, "td_box_pairs_ab_count: null pointer");
    if (td_status st = check_sets("td_box_pairs_ab_count", boxes_a, n_a, boxes_b, n_b)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TD_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_a, s));
    AbArgs A{};
    A.boxes_a = reinterpret_cast<const double2*>(boxes_a);
    A.boxes_b = reinterpret_cast<const double2*>(boxes_b);
    A.n_a = n_a;
    A.n_b = n_b;
    A.counts = counts;
    hipLaunchKernelGGL(box_pairs_ab_kernel<false>, ab_grid(n_a, n_b), dim3(AB_ROWS), 0, s, A);
    TD_KERNEL_CHECK();
    return TD_OK;
}

extern "C" td_status td_box_pairs_ab_fill(const double* boxes_a, int n_a, const double* boxes_b, int n_b, const int64_t* row_start,
                                          int32_t* cursor, int32_t* cols, void* stream) {
    TD_REQUIRE(boxes_a && boxes_b && row_start && cursor && cols, "td_box_pairs_ab_fill: null pointer");
    if (td_status st = check_sets("td_box_pairs_ab_fill", boxes_a, n_a, boxes_b, n_b)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TD_HIP_CHECK(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n_a, s));
    AbArgs A{};
    A.boxes_a = reinterpret_cast<const double2*>(boxes_a);
    A.boxes_b = reinterpret_cast<const double2*>(boxes_b);
    A.n_a = n_a;
    A.n_b = n_b;
    A.row_start = row_start;
    A.cursor = cursor;
    A.cols = cols;
    hipLaunchKernelGGL(box_pairs_ab_kernel<true>, ab_grid(n_a, n_b), dim3(AB_ROWS), 0, s, A);
    TD_KERNEL_CHECK();
    return TD_OK;
}
