// Intersection areas of polygon ring pairs (the polygon IoU of clean_crowns, reference TreeDetection/helpers.py:602-701 with
// utilities.calc_iou 209-212): for every listed pair (a ring of set A, a ring of set B) the exact-formula area of the
// intersection and the two ring areas. The arithmetic is ring_clip.h's, shared with the host twin (ringiou_host.cpp), which emulates
// the 64 lanes: the results are equal bit for bit.
//
// One wave per pair, RING_WPB waves per workgroup, each with a wave-private LDS region of RING_CAP vertices (x and y as two
// float64 arrays: 16 KiB per wave, 64 KiB per workgroup, two workgroups per CU of 160 KiB) that holds both rings as v - O. Nothing
// is shared between the waves of a workgroup, so there is no __syncthreads(): a wave orders its own LDS writes and reads with
// fences (TD_WAVE_SYNC). The lanes stride over the term index t = i * n + j, add their terms in ascending t and meet in a
// butterfly of __shfl_xor on doubles; lane 0 writes the pair's three results and its status. No atomics. The grid is bounded
// (RING_GRID_MAX workgroups) and a wave takes further pairs in a grid-stride loop: any number of pairs is one launch.
// status: 0 computed; 1 the two rings together have more than RING_CAP vertices — not computed (out is NaN), the host function
// serves such a pair; 2 refused — a pair index outside its ring set (no ring memory is touched), a ring of fewer than 3 vertices
// or a non-finite coordinate — out is NaN.
#include "common.h"
#include "ring_clip.h"
#include "wave_f64.h"

namespace {

constexpr int RING_WPB = 4;             // waves (pairs in flight) per workgroup
constexpr int RING_CAP = 1024;          // vertices of both rings of a pair that fit a wave's LDS region
constexpr int RING_GRID_MAX = 2048;     // workgroups of a launch: four rounds of the 2 x 256 that are resident at a time

// this wave's LDS writes before its later LDS reads: the fences of __syncthreads() without the s_barrier
#define TD_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); \
                           __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

struct RingLds {
    double x[RING_CAP];
    double y[RING_CAP];
};

// one ring into LDS as it lies in memory; → this lane's share of its bounding box, and whether a coordinate was not finite
__device__ __forceinline__ bool load_ring(const double* __restrict__ xy, int64_t first, int cnt, int lane, double* x, double* y, double* box) {
    const double2* v = reinterpret_cast<const double2*>(xy) + first;
    const double inf = __builtin_inf();
    box[0] = box[1] = inf;
    box[2] = box[3] = -inf;
    bool bad = false;
    for (int k = lane; k < cnt; k += 64) {
        const double2 p = v[k];
        bad |= !rc_finite(p.x) || !rc_finite(p.y);
        x[k] = p.x;
        y[k] = p.y;
        box[0] = p.x < box[0] ? p.x : box[0];
        box[1] = p.y < box[1] ? p.y : box[1];
        box[2] = p.x > box[2] ? p.x : box[2];
        box[3] = p.y > box[3] ? p.y : box[3];
    }
    box[0] = wave_min(box[0]);
    box[1] = wave_min(box[1]);
    box[2] = wave_max(box[2]);
    box[3] = wave_max(box[3]);
    return bad;
}

__global__ __launch_bounds__(64 * RING_WPB) void ring_pairs_kernel(const double* __restrict__ xy_a, const int64_t* __restrict__ start_a, int n_a,
                                                                   const double* __restrict__ xy_b, const int64_t* __restrict__ start_b, int n_b,
                                                                   const int32_t* __restrict__ pairs, int64_t n_pairs, double* __restrict__ out,
                                                                   int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) RingLds lds[RING_WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* const px = lds[wave].x;
    double* const py = lds[wave].y;
    for (int64_t p = (int64_t)blockIdx.x * RING_WPB + wave; p < n_pairs; p += (int64_t)gridDim.x * RING_WPB) {
        // everything up to the loads is the same in all 64 lanes
        const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
        int st = 0, m = 0, n = 0;
        int64_t a0 = 0, b0 = 0;
        if (ia < 0 || ia >= n_a || ib < 0 || ib >= n_b) {
            st = 2;
        } else {
            a0 = start_a[ia];
            b0 = start_b[ib];
            const int64_t ma = start_a[ia + 1] - a0, mb = start_b[ib + 1] - b0;
            if (a0 < 0 || b0 < 0 || ma < 3 || mb < 3) st = 2;
            else if (ma + mb > RING_CAP) st = 1;
            else m = (int)ma, n = (int)mb;
        }
        const double nan = __builtin_nan("");
        double res[3] = {nan, nan, nan};
        if (st == 0) {
            double* const qx = px + m;
            double* const qy = py + m;
            double ba[4], bb[4];
            TD_WAVE_SYNC();                              // the previous pair's reads are over
            bool bad = load_ring(xy_a, a0, m, lane, px, py, ba);
            bad |= load_ring(xy_b, b0, n, lane, qx, qy, bb);
            if (__any(bad)) {
                st = 2;
            } else {
                const double x0 = ba[0] > bb[0] ? ba[0] : bb[0], x1 = ba[2] < bb[2] ? ba[2] : bb[2];
                const double y0 = ba[1] > bb[1] ? ba[1] : bb[1], y1 = ba[3] < bb[3] ? ba[3] : bb[3];
                const double ox = (x0 + x1) / 2.0, oy = (y0 + y1) / 2.0;
                TD_WAVE_SYNC();
                for (int k = lane; k < m + n; k += 64) {  // (q follows p in the region)
                    px[k] = px[k] - ox;
                    py[k] = py[k] - oy;
                }
                TD_WAVE_SYNC();
                double sp = 0.0, sq = 0.0, acc = 0.0;
                for (int k = lane; k < m; k += 64) sp += rc_edge_cross(px, py, m, k);
                for (int k = lane; k < n; k += 64) sq += rc_edge_cross(qx, qy, n, k);
                sp = wave_sum(sp);
                sq = wave_sum(sq);
                if (x1 > x0 && y1 > y0) {
                    const int terms = m * n;             // <= (RING_CAP / 2)^2
                    for (int t = lane; t < terms; t += 64) {
                        const int i = t / n, j = t - i * n;
                        acc += rc_term(px, py, m, qx, qy, n, i, j);
                    }
                    acc = wave_sum(acc);
                }
                rc_finish(acc, sp, sq, res);
            }
        }
        if (lane == 0) {
            out[3 * p] = st == 0 ? res[0] : nan;
            out[3 * p + 1] = st == 0 ? res[1] : nan;
            out[3 * p + 2] = st == 0 ? res[2] : nan;
            status[p] = st;
        }
    }
}

}  // namespace

extern "C" td_status td_ring_pairs_area_dev(const double* xy_a, const int64_t* start_a, int n_a, const double* xy_b, const int64_t* start_b,
                                            int n_b, const int32_t* pairs, int64_t n_pairs, double* out, int32_t* status, void* stream) {
    TD_REQUIRE(xy_a && start_a && xy_b && start_b && pairs && out && status, "td_ring_pairs_area_dev: null pointer");
    TD_REQUIRE(n_a >= 0 && n_b >= 0, "td_ring_pairs_area_dev: n_a = %d, n_b = %d, ring counts cannot be negative", n_a, n_b);
    TD_REQUIRE(n_pairs >= 0, "td_ring_pairs_area_dev: n_pairs = %lld is negative", (long long)n_pairs);
    TD_REQUIRE(aligned16(xy_a) && aligned16(xy_b), "td_ring_pairs_area_dev: xy_a and xy_b must be 16-byte aligned (vertices are read as double2)");
    if (n_pairs == 0) return TD_OK;
    const int64_t groups = (n_pairs + RING_WPB - 1) / RING_WPB;
    const int grid = (int)(groups < RING_GRID_MAX ? groups : RING_GRID_MAX);
    hipLaunchKernelGGL(ring_pairs_kernel, dim3(grid), dim3(64 * RING_WPB), 0, static_cast<hipStream_t>(stream), xy_a, start_a, n_a, xy_b,
                       start_b, n_b, pairs, n_pairs, out, status);
    TD_KERNEL_CHECK();
    return TD_OK;
}
