// Per-crown raster statistics over the crown's OUTLINE: td_crown_zonal_dev, the opt-in alternative (config crown_statistics:
// polygon) to the bounding circles of td_crown_stats (crown.hip). Which pixels belong to a crown, the box searched for them and the
// order of the maximum and minimum are crown_zonal.h's, shared with the host twin (crownzonal_host.cpp), -ffp-contract=off on both
// sides: status, count, min, max and the position of the maximum are the host's bit for bit; mean and variance are float64 sums in
// another order, rounded once.
//
// One wave per crown, ZN_WPB waves per workgroup, a bounded grid with a grid-stride loop. The closed ring lies in a wave-private
// LDS region of TD_ZONAL_RING_CAP + 1 points; nothing is shared between waves, so there is no __syncthreads(): TD_WAVE_SYNC orders
// a wave's own LDS traffic. The wave walks the rows of crown_zonal.h's pixel box.
//   b == 0 and d == 0: P.y is one number along a row, so the row gets an active-edge list — the lanes stride over the edges, keep
//   those whose closed y-range holds P.y and compact their indices into LDS by ballot prefix; then a lane per pixel applies
//   query_edge_rule against the listed edges only. An edge outside the y-range answers 0 under that rule, so the verdict is
//   point_in_query's over all edges. Columns whose centre lies left of every listed edge's smallest x or right of the largest are
//   not walked: all listed edges are crossed, or none — an even number either way (the half-open rule lists every crossing of a
//   closed ring twice), and no envelope holds the point. (Only where the box is wider than one run of 64 pixels: within a run the
//   lanes wait for each other anyway.)
//   rotated: a lane per pixel of the box, point_in_query over the whole ring.
// Pass 1: count, sum (float64), minimum and maximum with their row-major positions, lanes joined by __shfl_xor butterflies (the
// orders of crown_zonal.h are total, so every lane ends with the same winner). Pass 2: the squared deviations from the float64
// mean — over the verdicts of pass 1, kept as one 64-bit mask per run of 64 pixels (ZN_RUNS of them in LDS; a crown with more
// runs, or a rotated transform, walks again). Lane 0 stores the crown's row with plain vector stores. All wave intrinsics sit in
// wave-uniform control flow.
//
// Reads: raster[row * cols + col] only for 0 <= row < rows, 0 <= col < cols (the box is clamped to the raster); xy only inside
// [start[q], start[q + 1]) after 0 <= start[q] <= start[q + 1] <= n_xy was checked — a wrong index gives status 2, not a load.
//
// td_crown_labels_dev, at the end of the file, is the same walk with a visitor that draws: the crown's value into a uint32 label
// raster by atomic maximum (the inverse question: which crown owns this pixel).
#include "common.h"
#include "crown_zonal.h"
#include "wave_f64.h"

namespace {

using namespace tdgeom;
using namespace tdzonal;

constexpr int ZN_WPB = 4;                // waves (crowns in flight) per workgroup
constexpr int ZN_GRID_MAX = 2048;        // workgroups of a launch
constexpr int ZN_CAP = TD_ZONAL_RING_CAP;
static_assert(ZN_CAP >= 256 && ZN_CAP < 65536, "the active-edge list holds 16-bit edge indices");

#define TD_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); \
                           __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

constexpr int ZN_RUNS = 256;             // runs of 64 pixels whose verdicts the wave keeps for the second pass

struct Run {
    long long base;                      // row * cols + first column: lane l stands for pixel base + l, in one raster row
    unsigned long long inside;           // bit l: that pixel belongs to the crown
};

struct ZonalLds {
    Pt ring[ZN_CAP + 1];                 // closed: ring[m] = ring[0]
    unsigned short active[ZN_CAP];       // the edges of the row in hand (edge j = ring[j] -> ring[j + 1])
    Run runs[ZN_RUNS];
};
static_assert(sizeof(ZonalLds) * ZN_WPB <= 64 * 1024, "static LDS of a workgroup");

struct ZonalArgs {
    const float* raster;
    int rows, cols;
    Affine t;
    const double2* xy;
    int64_t n_xy;
    const int64_t* start;
    int n;
    float* out;
    int32_t* pos;
    int32_t* status;
};

// Crown q's ring, checked and closed into L.ring[0 .. *m] → its status (0, 1 over ZN_CAP, 2 refused); with status 0 also its
// float64 bounding box, the same in every lane. start is checked before any vertex is read. (Args: ZonalArgs or LabelArgs.)
template <class Args>
__device__ __forceinline__ int ring_to_lds(const Args& A, ZonalLds& L, int64_t q, int lane, int* m_out, double* bx0, double* by0, double* bx1,
                                           double* by1) {
    const int64_t s = A.start[q], e = A.start[q + 1];
    int st = 0;
    if (s < 0 || e < s || e > A.n_xy || e - s < 3) st = 2;
    else if (e - s > ZN_CAP) st = 1;
    const int m = st == 0 ? (int)(e - s) : 0;
    const double inf = __builtin_inf();
    double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
    if (st == 0) {
        bool bad = false;
        TD_WAVE_SYNC();                                                // the previous crown's reads are over
        for (int k = lane; k <= m; k += 64) {
            const double2 p = A.xy[s + (k == m ? 0 : k)];
            bad |= !is_finite(p.x) || !is_finite(p.y);
            L.ring[k] = Pt{p.x, p.y};
            x0 = p.x < x0 ? p.x : x0;
            y0 = p.y < y0 ? p.y : y0;
            x1 = p.x > x1 ? p.x : x1;
            y1 = p.y > y1 ? p.y : y1;
        }
        TD_WAVE_SYNC();
        if (__any(bad)) st = 2;
    }
    if (st == 0) {
        x0 = wave_min(x0);
        y0 = wave_min(y0);
        x1 = wave_max(x1);
        y1 = wave_max(y1);
    }
    *m_out = m;
    *bx0 = x0;
    *by0 = y0;
    *bx1 = x1;
    *by1 = y1;
    return st;
}

// (Args: ZonalArgs, or LabelArgs below — the walk reads A.t and A.cols only.)
// visit(row, col) for every pixel of box B that belongs to the ring (L.ring[0 .. m], closed; bounding box x0 .. y1). The calls come
// from divergent lanes: visit holds no wave intrinsic. With `runs` the verdicts of the walk are kept: every run of 64 pixels with
// a pixel inside becomes an entry of L.runs, and *runs counts them — a count above ZN_RUNS says that the list is incomplete (the
// rotated walk, whose lanes do not share a row, always says so).
template <class Args, class Visit>
__device__ __forceinline__ void zonal_walk(const Args& A, ZonalLds& L, int m, const Box& B, double x0, double y0, double x1, double y1,
                                           int lane, int* runs, Visit&& visit) {
    if (runs) *runs = 0;
    if (B.r0 > B.r1 || B.c0 > B.c1) return;
    if (axis_aligned(A.t)) {
        const double inf = __builtin_inf();
        const bool wide = B.c1 - B.c0 >= 64;                           // more than one run per row: the listed edges' x-range can spare some
        for (int r = B.r0; r <= B.r1; ++r) {
            const double py = pixel_centre(A.t, r, B.c0).y;            // the same in every column
            if (py < y0 || py > y1) continue;
            TD_WAVE_SYNC();                                            // the previous row's reads of the list are over
            int na = 0;
            double ex0 = inf, ex1 = -inf;
            for (int base = 0; base < m; base += 64) {
                const int j = base + lane;
                bool keep = false;
                if (j < m) {
                    const Pt a = L.ring[j], b = L.ring[j + 1];
                    keep = py >= std::fmin(a.y, b.y) && py <= std::fmax(a.y, b.y);
                    if (keep) {
                        ex0 = std::fmin(ex0, std::fmin(a.x, b.x));
                        ex1 = std::fmax(ex1, std::fmax(a.x, b.x));
                    }
                }
                const unsigned long long mk = __ballot(keep);
                if (keep) L.active[na + __popcll(mk & ((1ull << lane) - 1))] = (unsigned short)j;
                na += __popcll(mk);
            }
            TD_WAVE_SYNC();
            if (na == 0) continue;
            int c0 = B.c0, c1 = B.c1;
            if (wide && A.t.a != 0.0) {
                int i0, i1;
                index_range(wave_min(ex0), wave_max(ex1), A.t.a, A.t.c, A.cols, &i0, &i1);
                c0 = i0 > c0 ? i0 : c0;
                c1 = i1 < c1 ? i1 : c1;
            }
            for (long long cb = c0; cb <= c1; cb += 64) {                // (64 bits: c1 may be the last int)
                bool in = false;
                if (cb + lane <= c1) {
                    const Pt P = pixel_centre(A.t, r, (int)(cb + lane));
                    bool on = false, odd = false;
                    for (int k = 0; k < na && !on; ++k) {
                        const int j = L.active[k];
                        const int code = query_edge_rule(L.ring[j], L.ring[j + 1], P);
                        on = code == 1;
                        odd ^= code == 2;
                    }
                    in = on || odd;
                }
                if (runs) {
                    const unsigned long long mk = __ballot(in);
                    if (mk) {
                        if (*runs < ZN_RUNS && lane == 0) L.runs[*runs] = Run{(long long)r * A.cols + cb, mk};
                        ++*runs;
                    }
                }
                if (in) visit(r, (int)(cb + lane));
            }
        }
        return;
    }
    if (runs) *runs = ZN_RUNS + 1;
    const int bw = B.c1 - B.c0 + 1, bh = B.r1 - B.r0 + 1;
    const long long total = (long long)bw * bh;
    for (long long p = lane; p < total; p += 64) {
        const int r = B.r0 + (int)(p / bw), col = B.c0 + (int)(p % bw);
        const Pt P = pixel_centre(A.t, r, col);
        if (in_bounds(P, x0, y0, x1, y1) && point_in_query(L.ring, m + 1, P) != 0) visit(r, col);
    }
}

__global__ __launch_bounds__(64 * ZN_WPB) void crown_zonal_kernel(const ZonalArgs A) {
    __shared__ __attribute__((aligned(16))) ZonalLds lds[ZN_WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ZonalLds& L = lds[wave];
    const float nanf_ = __builtin_nanf("");
    for (int64_t q = (int64_t)blockIdx.x * ZN_WPB + wave; q < A.n; q += (int64_t)gridDim.x * ZN_WPB) {
        int m;
        double x0, y0, x1, y1;
        const int st = ring_to_lds(A, L, q, lane, &m, &x0, &y0, &x1, &y1);
        float* o = A.out + 4 * q;
        int32_t* ps = A.pos + 3 * q;
        if (st != 0) {
            if (lane == 0) {
                o[0] = o[1] = o[2] = o[3] = nanf_;
                ps[0] = ps[1] = ps[2] = -1;
                A.status[q] = st;
            }
            continue;
        }
        const Box B = pixel_box(A.t, x0, y0, x1, y1, A.rows, A.cols);

        float vmax = 0.f, vmin = 0.f;
        long long imax = -1, imin = -1;
        int cnt = 0;
        double sum = 0.0;
        int runs = 0;
        zonal_walk(A, L, m, B, x0, y0, x1, y1, lane, &runs, [&](int r, int col) {
            const long long lin = (long long)r * A.cols + col;
            const float v = A.raster[lin];
            if (max_takes(v, lin, vmax, imax)) {
                vmax = v;
                imax = lin;
            }
            if (min_takes(v, lin, vmin, imin)) {
                vmin = v;
                imin = lin;
            }
            sum += (double)v;
            ++cnt;
        });
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(vmax, d), ow = __shfl_xor(vmin, d);
            const long long oi = __shfl_xor(imax, d), oj = __shfl_xor(imin, d);
            if (oi >= 0 && max_takes(ov, oi, vmax, imax)) {
                vmax = ov;
                imax = oi;
            }
            if (oj >= 0 && min_takes(ow, oj, vmin, imin)) {
                vmin = ow;
                imin = oj;
            }
            cnt += __shfl_xor(cnt, d);
        }
        sum = wave_sum(sum);
        if (cnt == 0) {
            if (lane == 0) {
                o[0] = o[1] = o[2] = o[3] = -1.f;
                ps[0] = 0;
                ps[1] = ps[2] = -1;
                A.status[q] = 0;
            }
            continue;
        }
        const double mean = sum / (double)cnt;
        double sq = 0.0;                                               // second pass: population variance about the float64 mean
        if (runs <= ZN_RUNS) {                                         // over the verdicts kept by the first pass
            TD_WAVE_SYNC();
            for (int k = 0; k < runs; ++k) {
                const Run run = L.runs[k];
                if ((run.inside >> lane) & 1) {
                    const double dv = (double)A.raster[run.base + lane] - mean;
                    sq += dv * dv;
                }
            }
        } else {                                                       // or over the same walk again
            zonal_walk(A, L, m, B, x0, y0, x1, y1, lane, nullptr, [&](int r, int col) {
                const double dv = (double)A.raster[(long long)r * A.cols + col] - mean;
                sq += dv * dv;
            });
        }
        sq = wave_sum(sq);
        if (lane == 0) {
            o[0] = vmin;
            o[1] = vmax;
            o[2] = (float)mean;
            o[3] = (float)(sq / (double)cnt);
            ps[0] = cnt;
            ps[1] = (int32_t)(imax / A.cols);
            ps[2] = (int32_t)(imax % A.cols);
            A.status[q] = 0;
        }
    }
}

// ---- td_crown_labels_dev: the same walk, drawing. labels[r][c] = max(labels[r][c], value[q]) for every pixel whose centre belongs to
// crown q: one relaxed agent-scope atomicMax per pixel inside, issued from the walk's visitor — on the axis-aligned path a run of 64
// pixels is one wave instruction over 256 contiguous bytes. The unsigned maximum does not depend on the order in which waves
// arrive, so the raster is the host twin's (crownlabels_host.cpp) bit for bit. No second pass, no `runs` list, nothing cleared.
// Writes: labels[row * cols + col] only for pixels of the box, which pixel_box clamps to the raster; status[q].
struct LabelArgs {
    int rows, cols;
    Affine t;
    const double2* xy;
    int64_t n_xy;
    const int64_t* start;
    const uint32_t* value;
    int n;
    unsigned* labels;
    int32_t* status;
};

__global__ __launch_bounds__(64 * ZN_WPB) void crown_labels_kernel(const LabelArgs A) {
    __shared__ __attribute__((aligned(16))) ZonalLds lds[ZN_WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ZonalLds& L = lds[wave];
    for (int64_t q = (int64_t)blockIdx.x * ZN_WPB + wave; q < A.n; q += (int64_t)gridDim.x * ZN_WPB) {
        int m;
        double x0, y0, x1, y1;
        const int st = ring_to_lds(A, L, q, lane, &m, &x0, &y0, &x1, &y1);
        if (lane == 0) A.status[q] = st;
        if (st != 0) continue;
        const unsigned v = A.value[q];
        if (v == 0u) continue;                                         // the maximum with 0 changes nothing
        const Box B = pixel_box(A.t, x0, y0, x1, y1, A.rows, A.cols);
        zonal_walk(A, L, m, B, x0, y0, x1, y1, lane, nullptr, [&](int r, int col) {
            __hip_atomic_fetch_max(A.labels + ((long long)r * A.cols + col), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
    }
}

}  // namespace

extern "C" td_status td_crown_labels_dev(int rows, int cols, const double* transform, const double* xy, int64_t n_xy, const int64_t* start,
                                         const uint32_t* value, int n, uint32_t* labels, int32_t* status, void* stream) {
    TD_REQUIRE(transform && xy && start && value && labels && status, "td_crown_labels_dev: null pointer");
    TD_REQUIRE(n >= 0 && n_xy >= 0, "td_crown_labels_dev: n = %d, n_xy = %lld, counts cannot be negative", n, (long long)n_xy);
    TD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols <= (int64_t)INT32_MAX,
               "td_crown_labels_dev: a %d x %d raster: both at least 1 and fewer than 2^31 pixels", rows, cols);
    for (int k = 0; k < 6; ++k)
        TD_REQUIRE(is_finite(transform[k]), "td_crown_labels_dev: transform[%d] is not finite", k);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(xy) % 16 == 0, "td_crown_labels_dev: xy must be 16-byte aligned (vertices are read as double2)");
    if (n == 0) return TD_OK;
    LabelArgs A{};
    A.rows = rows;
    A.cols = cols;
    A.t = Affine{transform[0], transform[1], transform[2], transform[3], transform[4], transform[5]};
    A.xy = reinterpret_cast<const double2*>(xy);
    A.n_xy = n_xy;
    A.start = start;
    A.value = value;
    A.n = n;
    A.labels = labels;
    A.status = status;
    const int64_t groups = ((int64_t)n + ZN_WPB - 1) / ZN_WPB;
    hipLaunchKernelGGL(crown_labels_kernel, dim3((unsigned)(groups < ZN_GRID_MAX ? groups : ZN_GRID_MAX)), dim3(64 * ZN_WPB), 0,
                       static_cast<hipStream_t>(stream), A);
    TD_KERNEL_CHECK();
    return TD_OK;
}

extern "C" td_status td_crown_zonal_dev(const float* raster, int rows, int cols, const double* transform, const double* xy, int64_t n_xy,
                                        const int64_t* start, int n, float* out, int32_t* pos, int32_t* status, void* stream) {
    TD_REQUIRE(raster && transform && xy && start && out && pos && status, "td_crown_zonal_dev: null pointer");
    TD_REQUIRE(n >= 0 && n_xy >= 0, "td_crown_zonal_dev: n = %d, n_xy = %lld, counts cannot be negative", n, (long long)n_xy);
    TD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols <= (int64_t)INT32_MAX,
               "td_crown_zonal_dev: a %d x %d raster: both at least 1 and fewer than 2^31 pixels (the count is an int32)", rows, cols);
    for (int k = 0; k < 6; ++k)
        TD_REQUIRE(is_finite(transform[k]), "td_crown_zonal_dev: transform[%d] is not finite", k);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(xy) % 16 == 0, "td_crown_zonal_dev: xy must be 16-byte aligned (vertices are read as double2)");
    if (n == 0) return TD_OK;
    ZonalArgs A{};
    A.raster = raster;
    A.rows = rows;
    A.cols = cols;
    A.t = Affine{transform[0], transform[1], transform[2], transform[3], transform[4], transform[5]};
    A.xy = reinterpret_cast<const double2*>(xy);
    A.n_xy = n_xy;
    A.start = start;
    A.n = n;
    A.out = out;
    A.pos = pos;
    A.status = status;
    const int64_t groups = ((int64_t)n + ZN_WPB - 1) / ZN_WPB;
    hipLaunchKernelGGL(crown_zonal_kernel, dim3((unsigned)(groups < ZN_GRID_MAX ? groups : ZN_GRID_MAX)), dim3(64 * ZN_WPB), 0,
                       static_cast<hipStream_t>(stream), A);
    TD_KERNEL_CHECK();
    return TD_OK;
}
