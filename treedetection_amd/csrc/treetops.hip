// Treetops in a height raster: td_treetops_dev. One launch; a workgroup of 256 lanes owns a T x T output tile (T = 64, or 32 when
// the halo would not fit 64 KB of LDS) and keeps everything between the raw raster and the marks in LDS:
//   1. the raw tile with its halo of H = r + h pixels, E = T + 2H on a side, into buffer A — coalesced row loads, the reflect rule of
//      treetops.h applied to the global index at the load (so the staged tile IS the reflected extension, however far it reaches);
//   2. the axis-0 pass A -> B: E0 = T + 2h rows of E columns;   3. the axis-1 pass B -> A: E0 x E0, the smoothed tile with its halo h;
//   4. the maximum down the columns A -> B: T rows of E0 columns;   5. per output pixel the maximum along the row of B, the comparison
//      with its own smoothed value in A, and the stores straight from registers: marks, smoothed, one atomic add per tile row.
// The smoothed halo beyond the raster's edge holds the smoothed values of the reflected extension, which are the mirror images of
// smoothed values inside the window already (the extension is symmetric about the edge and the pass adds the pair l + ii, l - ii
// commutatively): taking them into the maximum changes nothing, so the window needs no range test. Both passes and the maximum use the
// functions of treetops.h, in float64 with -ffp-contract=off: marks and smoothed are the host twin's (treetops_host.cpp) bit for bit.
// LDS: in every stage consecutive lanes read and write consecutive dwords of a row (the flat element index runs along the row), so the
// column pass is as conflict-free as the row pass; 2 * E * E * 4 bytes, 43 808 for the defaults (r = 2, h = 3, T = 64, E = 74).
// Writes: marks / smoothed [row * cols + col] only for row < rows and col < cols; counts[row] only for row < rows.
#include "common.h"
#include "treetops.h"

using namespace tdtops;

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_LDS_BYTES = 64 * 1024;
constexpr unsigned TT_GRID_MAX = 1u << 20;                         // workgroups of one launch; a larger raster's tiles are walked in a grid-stride loop

struct TopsArgs {
    const float* raster;
    int rows, cols;
    int r, h;
    float floor;
    uint8_t* marks;
    float* smoothed;
    int32_t* counts;
    unsigned tiles_x, tiles;                                       // tiles along a row of tiles and all of them: a bounded 1-D grid walks them
    double w[2 * TD_TREETOP_RADIUS_CAP + 1];
};

// floor(i / d) for i * d < 2^32 by one multiply: magic = floor((2^32 - 1) / d) + 1
__device__ inline unsigned div_by(unsigned i, unsigned magic) { return __umulhi(i, magic); }

template <int T>
__global__ __launch_bounds__(TT_THREADS) void treetops_kernel(const TopsArgs A) {
    extern __shared__ float lds[];
    const int r = A.r, h = A.h, H = r + h;
    const int E = T + 2 * H, E0 = T + 2 * h;                       // E <= 90: every flat index below is under 2^13
    float* const bufA = lds;
    float* const bufB = lds + E * E;
    const unsigned magicE = 0xFFFFFFFFu / (unsigned)E + 1u, magicE0 = 0xFFFFFFFFu / (unsigned)E0 + 1u;
    const int tid = threadIdx.x;
    for (unsigned tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {      // (uniform: the barriers below are met by all)
        const unsigned tile_y = tile / A.tiles_x, tile_x = tile - tile_y * A.tiles_x;
        const long long row0 = (long long)tile_y * T, col0 = (long long)tile_x * T;            // the tile's first output pixel

        // 1. raw tile + halo: A[y][x] = raster[reflect(row0 - H + y)][reflect(col0 - H + x)]
        for (int i = tid; i < E * E; i += TT_THREADS) {
            const int y = (int)div_by(i, magicE), x = i - y * E;
            const int gr = reflect(row0 - H + y, A.rows), gc = reflect(col0 - H + x, A.cols);
            bufA[i] = A.raster[(size_t)gr * A.cols + gc];
        }
        __syncthreads();
        // 2. axis 0: B[y][x] = pass over A[y + r + ii][x], y < E0, x < E
        for (int i = tid; i < E0 * E; i += TT_THREADS) {
            const float* centre = bufA + i + r * E;
            bufB[i] = smooth_one(A.w, r, [&](int ii) { return centre[ii * E]; });
        }
        __syncthreads();
        // 3. axis 1: A[y][x] = pass over B[y][x + r + ii], y < E0, x < E0 (pitch E0)
        for (int i = tid; i < E0 * E0; i += TT_THREADS) {
            const int y = (int)div_by(i, magicE0), x = i - y * E0;
            const float* centre = bufB + y * E + x + r;
            bufA[i] = smooth_one(A.w, r, [&](int ii) { return centre[ii]; });
        }
        __syncthreads();
        // 4. the maximum down the columns: B[y][x] = fmax_nan over A[y .. y + 2h][x], y < T, x < E0 (pitch E0)
        for (int i = tid; i < T * E0; i += TT_THREADS) {
            float m = bufA[i];
            for (int q = 1; q <= 2 * h; ++q) m = fmax_nan(m, bufA[i + q * E0]);
            bufB[i] = m;
        }
        __syncthreads();
        // 5. along the rows, the comparison, the stores: a wave covers 64 / T tile rows per step, a lane one pixel
        constexpr int ROWS_PER_STEP = TT_THREADS / T;
        const int x = tid % T, ysub = tid / T;
        const long long gc = col0 + x;
        for (int y = ysub; y < T; y += ROWS_PER_STEP) {
            const long long gr = row0 + y;                                  // (uniform over the lanes that share a tile row)
            const float* line = bufB + y * E0 + x;
            float m = line[0];
            for (int q = 1; q <= 2 * h; ++q) m = fmax_nan(m, line[q]);
            const float s = bufA[(y + h) * E0 + x + h];
            const bool inside = gr < A.rows && gc < A.cols;
            const bool top = inside && is_top(s, m, A.floor);
            if (inside) {
                const size_t at = (size_t)gr * A.cols + (size_t)gc;
                A.marks[at] = top ? 1 : 0;
                if (A.smoothed) A.smoothed[at] = s;
            }
            if (A.counts) {                                                 // (uniform: every lane votes)
                const unsigned long long votes = __ballot(top);
                const int sub = (tid & 63) / T;                             // which of the wave's tile rows this lane is in
                const unsigned long long mine = T == 64 ? votes : (votes >> (sub * T)) & ((1ull << (T & 63)) - 1ull);
                const int tops = __popcll(mine);
                if ((tid & 63) % T == 0 && tops > 0 && gr < A.rows)
                    __hip_atomic_fetch_add(A.counts + gr, tops, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                                                // the next tile's loads overwrite what step 5 read
    }
}

}  // namespace

extern "C" td_status td_treetops_dev(const float* raster, int rows, int cols, const double* weights, int radius, int window, float floor,
                                     uint8_t* marks, float* smoothed, int32_t* counts, void* stream) {
    TD_REQUIRE(raster && weights && marks, "td_treetops_dev: null pointer");
    TD_REQUIRE(radius <= TD_TREETOP_RADIUS_CAP && window <= TD_TREETOP_WINDOW_CAP,
               "td_treetops_dev: radius %d, window %d: the kernel holds a radius up to %d and a window up to %d (td_treetops has no cap)", radius,
               window, TD_TREETOP_RADIUS_CAP, TD_TREETOP_WINDOW_CAP);
    if (const char* why = refusal(rows, cols, weights, radius, window, floor)) {
        td_set_error("td_treetops_dev: %s (a %d x %d raster, radius %d, window %d)", why, rows, cols, radius, window);
        return TD_ERR_INVALID;
    }
    TopsArgs A{};
    A.raster = raster;
    A.rows = rows;
    A.cols = cols;
    A.r = radius;
    A.h = window / 2;
    A.floor = floor;
    A.marks = marks;
    A.smoothed = smoothed;
    A.counts = counts;
    for (int i = 0; i <= 2 * radius; ++i) A.w[i] = weights[i];
    const int H = A.r + A.h;
    const int T = 64 + 2 * H <= 90 ? 64 : 32;                            // 2 * E * E * 4 <= 64 KB needs E <= 90
    const int E = T + 2 * H;
    const size_t lds_bytes = (size_t)2 * E * E * sizeof(float);
    TD_REQUIRE(lds_bytes <= (size_t)TT_LDS_BYTES, "td_treetops_dev: %zu bytes of LDS for radius %d, window %d", lds_bytes, radius, window);
    const int64_t gx = ((int64_t)cols + T - 1) / T, gy = ((int64_t)rows + T - 1) / T;      // gx * gy < 2^31 / 32^2 + (rows + cols) / 32 + 1
    A.tiles_x = (unsigned)gx;
    A.tiles = (unsigned)(gx * gy);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (counts) TD_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)rows * sizeof(int32_t), s));
    const dim3 grid(A.tiles < TT_GRID_MAX ? A.tiles : TT_GRID_MAX);
    if (T == 64)
        hipLaunchKernelGGL(treetops_kernel<64>, grid, dim3(TT_THREADS), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(treetops_kernel<32>, grid, dim3(TT_THREADS), lds_bytes, s, A);
    TD_KERNEL_CHECK();
    return TD_OK;
}
