// Outline predicates on the device: td_region_relate_dev, the twin of td_region_relate (region.cpp) for many query rings against
// one packed region. Same definitions (region.cpp's header comment), same arithmetic (geom_predicates.h, -ffp-contract=off): every
// orientation sign is exact and every meeting parameter and piece midpoint is formed by the operations of the host function, so the
// flags are equal to the host's whatever the order in which edges are visited here.
//
// Index: the host's y-bins as two flat arrays (bin_start [n_bins + 1], bin_edges: the edge ids of a bin in ascending order, an edge
// in every bin its y-range touches). Edge id = index of its first vertex in ring_xy; edge_ring [n_vertices] names the ring of a
// vertex, so an edge brings its endpoints, ring and polygon without a table of its own.
//
// One wave per query, RR_WPB waves per workgroup, a bounded grid with a grid-stride loop. The query's vertices, the meeting
// parameters of the edge in hand and the rings met so far live in a wave-private LDS region of fixed capacity (TD_RELATE_*_CAP,
// include/treedet.h); nothing is shared between waves, so there is no __syncthreads(): TD_WAVE_SYNC orders a wave's own LDS
// traffic. The 64 lanes stride over the edges of a bin: membership of a point (vertex, piece midpoint, first vertex of a hole) is
// one pass over the bin of its y, with the per-polygon parity taken from ballots (the edge ids of a bin ascend, so the crossings
// of one polygon are neighbours); the region edges whose envelope meets the query's box are listed once per query (RR_CCAP ids in
// LDS; when there are more, every pass walks the bins of the query's y-range instead, an edge counted in the first of those bins
// it lies in — same edges, no capacity), and the meetings of one query edge are one pass over them. All control flow is the same in the 64 lanes. No atomics: lane 0 writes
// flags[q] and status[q] with plain stores once the query is decided.
//
// status 0 decided; 1 not decided (flag 0): more vertices than TD_RELATE_QUERY_CAP, more meetings on one query edge than
// TD_RELATE_MEET_CAP while `within` was still open, or more distinct region rings met than TD_RELATE_RING_CAP — td_region_relate
// decides such a query; 2 refused (flag 0): fewer than 4 points, not closed, a non-finite coordinate, a start outside the vertices.
// Every id read from the index is checked against the array sizes before it addresses anything; a bin range is clamped to the edge
// list. What an inconsistent index does to the ANSWER is not defined, which is why the entry point can check one first.
#include "common.h"
#include "geom_predicates.h"
#include "wave_f64.h"

namespace {

using namespace tdgeom;

constexpr int RR_WPB = 4;               // waves (queries in flight) per workgroup
constexpr int RR_GRID_MAX = 4096;       // workgroups of a launch
constexpr int RR_QCAP = TD_RELATE_QUERY_CAP;
constexpr int RR_MCAP = TD_RELATE_MEET_CAP;
constexpr int RR_RCAP = TD_RELATE_RING_CAP;
constexpr int RR_CCAP = 1024;           // region edges near a query that the wave lists in LDS; more are walked from the bins each time
static_assert(RR_RCAP <= 64, "the met-ring list is searched with one compare per lane");

#define TD_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); \
                           __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

struct Rel {
    const double2* xy;
    const int64_t* ring_start;
    const int32_t* ring_poly;
    const int32_t* edge_ring;
    const int32_t* bin_start;
    const int32_t* bin_edges;
    int n_rings, n_vertices, n_bins, n_bin_edges;
    double ymin, ymax, inv_h;
};

struct RelLds {
    double qx[RR_QCAP];
    double qy[RR_QCAP];
    double ts[RR_MCAP + 2];
    double sorted[RR_MCAP + 2];
    int met[RR_RCAP];
    int cand[RR_CCAP];
};

__device__ __forceinline__ bool rr_finite(double v) { return v - v == 0.0; }

__device__ __forceinline__ int bin_of(const Rel& R, double y) { return relate_bin_of(y, R.ymin, R.inv_h, R.n_bins); }

// the slice of bin_edges that bin b (0 <= b < n_bins) names, clamped to the list
__device__ __forceinline__ void bin_range(const Rel& R, int b, int* s, int* e) {
    const int s0 = R.bin_start[b], e0 = R.bin_start[b + 1];
    *s = s0 < 0 ? 0 : s0;
    *e = e0 > R.n_bin_edges ? R.n_bin_edges : e0;
}

// an edge id from the index: may its two vertices and its ring be read?
__device__ __forceinline__ bool edge_of(const Rel& R, int id, int* ring) {
    if (id < 0 || id >= R.n_vertices - 1) return false;
    const int r = R.edge_ring[id];
    if (r < 0 || r >= R.n_rings) return false;
    *ring = r;
    return true;
}
__device__ __forceinline__ Pt vertex(const Rel& R, int id) {
    const double2 v = R.xy[id];
    return {v.x, v.y};
}

// Region::classify + "some polygon has p": p on a ring of a polygon, or an odd crossing count for a polygon — polygons other than
// `skip_poly` only when `skip` (the "hole covered by another polygon" rule). The same answer in all lanes.
__device__ bool member(const Rel& R, const Pt& p, bool skip, int skip_poly, int lane) {
    if (p.y < R.ymin || p.y > R.ymax) return false;
    int s, e;
    bin_range(R, bin_of(R, p.y), &s, &e);
    bool found = false, have = false;
    int cur_poly = 0, cur_par = 0;
    for (int base = s; base < e && !found; base += 64) {
        const int k = base + lane;
        int code = 0, poly = 0, ring;
        if (k < e) {
            const int id = R.bin_edges[k];
            if (edge_of(R, id, &ring)) {
                poly = R.ring_poly[ring];
                code = edge_point_rule(vertex(R, id), vertex(R, id + 1), p);
            }
        }
        const bool counts = !skip || poly != skip_poly;
        if (__any(code == 1 && counts)) return true;
        unsigned long long m = __ballot(code == 2);
        while (m) {
            const int P = __shfl(poly, __ffsll((long long)m) - 1);
            const unsigned long long mine = __ballot(code == 2 && poly == P);
            m &= ~mine;
            if (!have || P != cur_poly) {
                if (have && cur_par && !(skip && cur_poly == skip_poly)) found = true;
                have = true;
                cur_poly = P;
                cur_par = 0;
            }
            cur_par ^= __popcll(mine) & 1;
        }
    }
    if (have && cur_par && !(skip && cur_poly == skip_poly)) found = true;
    return found;
}

// The region edges near a query — those whose envelope meets the query's box — a round of 64 at a time: from the wave's LDS list when
// they fitted it (collected once per query, as the host function collects its candidates), else straight from the bins of the
// query's y-range, an edge taken in the first of those bins it lies in. The cursor is the same in all lanes.
struct Walk {
    bool listed;
    int ncand, b0, b1;
    double x0, y0, x1, y1;
    int b, pos, end;
};
__device__ __forceinline__ void walk_start(Walk& w) {
    w.b = w.b0 - 1;
    w.pos = 0;
    w.end = w.listed ? w.ncand : 0;
}
// → false when the edges are exhausted; else *ok says whether this lane holds one (id, its ring, its endpoints) in this round
__device__ __forceinline__ bool walk_next(const Rel& R, const RelLds& L, Walk& w, int lane, bool* ok, int* id, int* ring, Pt* a, Pt* c) {
    *ok = false;
    if (w.listed) {
        if (w.pos >= w.end) return false;
        const int k = w.pos + lane;
        w.pos += 64;
        if (k < w.end) {
            *id = L.cand[k];
            if (edge_of(R, *id, ring)) {
                *a = vertex(R, *id);
                *c = vertex(R, *id + 1);
                *ok = true;
            }
        }
        return true;
    }
    while (w.pos >= w.end) {
        if (++w.b > w.b1) return false;
        bin_range(R, w.b, &w.pos, &w.end);
    }
    const int k = w.pos + lane;
    w.pos += 64;
    if (k < w.end) {
        *id = R.bin_edges[k];
        if (edge_of(R, *id, ring)) {
            *a = vertex(R, *id);
            *c = vertex(R, *id + 1);
            const int first = bin_of(R, std::fmin(a->y, c->y));              // the edge's first bin: it is taken once,
            const bool here = (first > w.b0 ? first : w.b0) == w.b;          // in the first bin of the query it lies in
            const bool close_by = !(std::fmax(a->x, c->x) < w.x0 || std::fmin(a->x, c->x) > w.x1 || std::fmax(a->y, c->y) < w.y0 ||
                                    std::fmin(a->y, c->y) > w.y1);
            *ok = here && close_by;
        }
    }
    return true;
}

// → status (0 / 1); *flags_out the two bits. Q = L.qx / L.qy [n], closed, finite, its box (x0, y0, x1, y1) meets the region in y.
__device__ int relate_one(const Rel& R, RelLds& L, int n, double x0, double y0, double x1, double y1, int lane, unsigned* flags_out) {
    bool inter = false, within = true;
    // (1) vertices
    for (int i = 0; i + 1 < n; ++i) {
        const Pt p{L.qx[i], L.qy[i]};
        if (member(R, p, false, 0, lane)) inter = true;
        else within = false;
        if (inter && !within) break;
    }
    if (inter && !within) {                              // decided: nothing below can change either flag
        *flags_out = 1u;
        return 0;
    }
    Walk w{false, 0, bin_of(R, y0), bin_of(R, y1), x0, y0, x1, y1, 0, 0, 0};
    bool ok;
    int id = 0, ring = 0;
    Pt a{0.0, 0.0}, c{0.0, 0.0};
    {   // the edges near the query into the list, if they fit
        int ncand = 0;
        bool fits = true;
        walk_start(w);
        while (fits && walk_next(R, L, w, lane, &ok, &id, &ring, &a, &c)) {
            const unsigned long long m = __ballot(ok);
            if (ncand + __popcll(m) > RR_CCAP) fits = false;
            else {
                if (ok) L.cand[ncand + __popcll(m & ((1ull << lane) - 1))] = id;
                ncand += __popcll(m);
            }
        }
        TD_WAVE_SYNC();
        w.listed = fits;
        w.ncand = ncand;
    }
    // (2) edges: meetings with region edges, then the pieces between them
    int nmet = 0;
    for (int i = 0; i + 1 < n; ++i) {
        if (inter && !within) break;                     // decided: flags = intersects only
        const Pt A{L.qx[i], L.qy[i]}, B{L.qx[i + 1], L.qy[i + 1]};
        int cnt = 0;
        TD_WAVE_SYNC();                                  // the previous edge's reads of ts / sorted are over
        walk_start(w);
        while (walk_next(R, L, w, lane, &ok, &id, &ring, &a, &c)) {
            int nm = 0;
            double t[2] = {0.0, 0.0};
            if (ok) nm = meet_params(A, B, a, c, t);
            const unsigned long long m1 = __ballot(nm >= 1);
            if (!m1) continue;
            inter = true;
            if (!within) continue;
            unsigned long long pend = m1;                                        // the rings met, each once
            while (pend) {
                const int r = __shfl(ring, __ffsll((long long)pend) - 1);
                pend &= ~__ballot(nm >= 1 && ring == r);
                if (__any(lane < nmet && L.met[lane] == r)) continue;
                if (nmet == RR_RCAP) return 1;
                if (lane == 0) L.met[nmet] = r;
                ++nmet;
                TD_WAVE_SYNC();
            }
            const unsigned long long m2 = __ballot(nm == 2), below = (1ull << lane) - 1;
            const int total = __popcll(m1) + __popcll(m2);
            if (cnt + total > RR_MCAP) return 1;
            const int off = cnt + __popcll(m1 & below) + __popcll(m2 & below);
            if (nm >= 1) L.ts[off] = t[0];
            if (nm == 2) L.ts[off + 1] = t[1];
            cnt += total;
        }
        if (!within) continue;
        if (lane == 0) {
            L.ts[cnt] = 0.0;
            L.ts[cnt + 1] = 1.0;
        }
        cnt += 2;
        TD_WAVE_SYNC();
        for (int k = lane; k < cnt; k += 64) {           // rank sort: equal values keep their order, every slot is written once
            const double v = L.ts[k];
            int rank = 0;
            for (int j = 0; j < cnt; ++j) {
                const double u = L.ts[j];
                rank += (u < v || (u == v && j < k)) ? 1 : 0;
            }
            L.sorted[rank] = v;
        }
        TD_WAVE_SYNC();
        for (int j = 0; j + 1 < cnt; ++j) {
            const double t0 = L.sorted[j], t1 = L.sorted[j + 1];
            if (!(t1 > t0)) continue;
            if (!member(R, piece_midpoint(A, B, t0, t1), false, 0, lane)) {
                within = false;
                break;
            }
        }
    }
    // (3) region rings lying loose inside the query: the first edge of such a ring is one of the edges near the query
    if (!inter || within) {
        walk_start(w);
        while ((!inter || within) && walk_next(R, L, w, lane, &ok, &id, &ring, &a, &c)) {
            const bool cand = ok && R.ring_start[ring] == (int64_t)id && !(a.x < x0 || a.x > x1 || a.y < y0 || a.y > y1);
            unsigned long long pend = __ballot(cand);
            while (pend && (!inter || within)) {
                const int src = __ffsll((long long)pend) - 1;
                pend &= pend - 1;
                const int r = __shfl(ring, src);
                const Pt f{__shfl(a.x, src), __shfl(a.y, src)};
                if (__any(lane < nmet && L.met[lane] == r)) continue;
                bool on = false, odd = false;            // point_in_query, an edge per lane
                for (int i = lane; i + 1 < n; i += 64) {
                    const int q = query_edge_rule(Pt{L.qx[i], L.qy[i]}, Pt{L.qx[i + 1], L.qy[i + 1]}, f);
                    on |= q == 1;
                    odd ^= q == 2;
                }
                if (!__any(on) && !(__popcll(__ballot(odd)) & 1)) continue;
                inter = true;
                const int poly = R.ring_poly[r];
                if (within && r > 0 && R.ring_poly[r - 1] == poly) {
                    // the hole is open ground unless a polygon other than its own has its first vertex
                    if (!member(R, f, true, poly, lane)) within = false;
                }
            }
        }
    }
    *flags_out = (inter ? 1u : 0u) | ((inter && within) ? 2u : 0u);
    return 0;
}

__global__ __launch_bounds__(64 * RR_WPB) void region_relate_kernel(Rel R, const double2* __restrict__ qxy, const int64_t* __restrict__ qstart,
                                                                    int n_queries, int64_t n_qvertices, uint8_t* __restrict__ flags,
                                                                    int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) RelLds lds[RR_WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RelLds& L = lds[wave];
    for (int64_t q = (int64_t)blockIdx.x * RR_WPB + wave; q < n_queries; q += (int64_t)gridDim.x * RR_WPB) {
        const int64_t s = qstart[q], e = qstart[q + 1];
        int st = 0;
        unsigned fl = 0;
        if (s < 0 || e > n_qvertices || e - s < 4) st = 2;
        else if (e - s > RR_QCAP) st = 1;
        if (st == 0) {
            const int n = (int)(e - s);
            const double inf = __builtin_inf();
            double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
            bool bad = false;
            TD_WAVE_SYNC();                              // the previous query's reads are over
            for (int k = lane; k < n; k += 64) {
                const double2 p = qxy[s + k];
                bad |= !rr_finite(p.x) || !rr_finite(p.y);
                L.qx[k] = p.x;
                L.qy[k] = p.y;
                x0 = p.x < x0 ? p.x : x0;
                y0 = p.y < y0 ? p.y : y0;
                x1 = p.x > x1 ? p.x : x1;
                y1 = p.y > y1 ? p.y : y1;
            }
            TD_WAVE_SYNC();
            x0 = wave_min(x0);
            y0 = wave_min(y0);
            x1 = wave_max(x1);
            y1 = wave_max(y1);
            const bool closed = L.qx[0] == L.qx[n - 1] && L.qy[0] == L.qy[n - 1];
            if (__any(bad) || !closed) st = 2;
            else if (!(y1 < R.ymin || y0 > R.ymax)) st = relate_one(R, L, n, x0, y0, x1, y1, lane, &fl);   // else disjoint in y: 0
        }
        if (lane == 0) {
            flags[q] = st == 0 ? (uint8_t)fl : (uint8_t)0;
            status[q] = st;
        }
    }
}

// ---- the index against the arrays it points into: one thread per entry of the longest array; *verdict collects the BAD_* bits
enum { BAD_BIN_START = 1, BAD_EDGE_ID = 2, BAD_EDGE_RING = 4, BAD_POLY_ORDER = 8, BAD_BIN_ORDER = 16 };

__global__ void region_index_check_kernel(Rel R, int32_t* verdict) {
    const int64_t n = (int64_t)blockDim.x * gridDim.x;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= R.n_bins || i < R.n_bin_edges || i < R.n_rings; i += n) {
        if (i <= R.n_bins) {
            const int s = R.bin_start[i];
            if (s < 0 || s > R.n_bin_edges) bad |= BAD_BIN_START;
            if (i < R.n_bins) {
                const int e = R.bin_start[i + 1];
                if (e < s) bad |= BAD_BIN_START;
                else if (s >= 0 && e <= R.n_bin_edges)
                    for (int k = s; k + 1 < e; ++k)
                        if (R.bin_edges[k + 1] <= R.bin_edges[k]) bad |= BAD_BIN_ORDER;
            }
        }
        if (i < R.n_bin_edges) {
            const int id = R.bin_edges[i];
            if (id < 0 || id >= R.n_vertices - 1) bad |= BAD_EDGE_ID;
            else {
                const int r = R.edge_ring[id];
                if (r < 0 || r >= R.n_rings) bad |= BAD_EDGE_RING;
                else if ((int64_t)id < R.ring_start[r] || (int64_t)id + 1 >= R.ring_start[r + 1]) bad |= BAD_EDGE_RING;
            }
        }
        if (i + 1 < R.n_rings && R.ring_poly[i + 1] < R.ring_poly[i]) bad |= BAD_POLY_ORDER;
    }
    if (bad) atomicOr(verdict, bad);
}

}  // namespace

extern "C" td_status td_region_relate_dev(const double* ring_xy, const int64_t* ring_start, const int32_t* ring_poly, int n_rings,
                                          int64_t n_vertices, const int32_t* edge_ring, const int32_t* bin_start, const int32_t* bin_edges,
                                          int n_bins, int64_t n_bin_edges, double ymin, double ymax, double inv_h, const double* query_xy,
                                          const int64_t* query_start, int n_queries, int64_t n_query_vertices, uint8_t* flags,
                                          int32_t* status, int check_index, void* stream) {
    TD_REQUIRE(ring_xy && ring_start && ring_poly && edge_ring && bin_start && bin_edges && query_xy && query_start && flags && status,
               "td_region_relate_dev: null pointer");
    TD_REQUIRE(n_rings >= 1 && n_vertices >= 4 && n_vertices < (int64_t)INT32_MAX,
               "td_region_relate_dev: n_rings = %d, n_vertices = %lld: a region has a ring and fewer than 2^31 - 1 vertices", n_rings,
               (long long)n_vertices);
    TD_REQUIRE(n_bins >= 1 && n_bin_edges >= 0 && n_bin_edges < (int64_t)INT32_MAX,
               "td_region_relate_dev: n_bins = %d, n_bin_edges = %lld: an index has a bin and fewer than 2^31 - 1 entries", n_bins,
               (long long)n_bin_edges);
    TD_REQUIRE(n_queries >= 0 && n_query_vertices >= 0, "td_region_relate_dev: n_queries = %d, n_query_vertices = %lld, counts cannot be negative",
               n_queries, (long long)n_query_vertices);
    TD_REQUIRE(ymin - ymin == 0.0 && ymax - ymax == 0.0 && ymin <= ymax && inv_h - inv_h == 0.0 && inv_h >= 0.0,
               "td_region_relate_dev: ymin, ymax, inv_h must be finite with ymin <= ymax and inv_h >= 0");
    TD_REQUIRE(aligned16(ring_xy) && aligned16(query_xy), "td_region_relate_dev: ring_xy and query_xy must be 16-byte aligned (vertices are read as double2)");
    if (n_queries == 0) return TD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Rel R{reinterpret_cast<const double2*>(ring_xy), ring_start, ring_poly, edge_ring, bin_start, bin_edges, n_rings, (int)n_vertices,
                n_bins, (int)n_bin_edges, ymin, ymax, inv_h};
    if (check_index) {
        // status[0] is the verdict word until the relate kernel overwrites it
        TD_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
        int64_t longest = (int64_t)n_bins + 1;
        longest = n_bin_edges > longest ? n_bin_edges : longest;
        longest = n_rings > longest ? n_rings : longest;
        const int64_t groups = (longest + 255) / 256;
        hipLaunchKernelGGL(region_index_check_kernel, dim3((unsigned)(groups < 4096 ? groups : 4096)), dim3(256), 0, s, R, status);
        TD_KERNEL_CHECK();
        int32_t verdict = 0;
        TD_HIP_CHECK(hipMemcpyAsync(&verdict, status, sizeof verdict, hipMemcpyDeviceToHost, s));
        TD_HIP_CHECK(hipStreamSynchronize(s));
        TD_REQUIRE(!(verdict & BAD_BIN_START), "td_region_relate_dev: bin_start does not rise from >= 0 to <= n_bin_edges = %lld", (long long)n_bin_edges);
        TD_REQUIRE(!(verdict & BAD_EDGE_ID), "td_region_relate_dev: a bin_edges entry points past the edge array (edge ids are 0 .. %lld)",
                   (long long)n_vertices - 2);
        TD_REQUIRE(!(verdict & BAD_EDGE_RING), "td_region_relate_dev: edge_ring does not name the ring whose vertices hold the edge");
        TD_REQUIRE(!(verdict & BAD_POLY_ORDER), "td_region_relate_dev: ring_poly must not decrease");
        TD_REQUIRE(!(verdict & BAD_BIN_ORDER), "td_region_relate_dev: the edge ids of a bin must ascend");
    }
    const int64_t groups = ((int64_t)n_queries + RR_WPB - 1) / RR_WPB;
    hipLaunchKernelGGL(region_relate_kernel, dim3((unsigned)(groups < RR_GRID_MAX ? groups : RR_GRID_MAX)), dim3(64 * RR_WPB), 0, s, R,
                       reinterpret_cast<const double2*>(query_xy), query_start, n_queries, n_query_vertices, flags, status);
    TD_KERNEL_CHECK();
    return TD_OK;
}
