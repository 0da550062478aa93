// The host twin of td_crown_zonal_dev (crownzonal.hip): membership, box and the orders of maximum and minimum from the same header
// (crown_zonal.h), so status, count, min, max and the position of the maximum equal the device's bit for bit. It states the
// definition directly — point_in_query over ALL edges of the ring for every pixel of the box, in row-major order, no active-edge
// list — and has no vertex cap: it serves the crowns the kernel marks status 1, the host path of crown_zonal_stats (device=None)
// and the CPU tests. Mean and variance: float64 sums in row-major order, the variance in a second pass about the float64 mean, each
// rounded once. Host code.
#include "common.h"
#include "crown_zonal.h"

#include <limits>
#include <vector>

using namespace tdzonal;

extern "C" td_status td_crown_zonal(const float* raster, int rows, int cols, const double* transform, const double* xy, int64_t n_xy,
                                    const int64_t* start, int n, float* out, int32_t* pos, int32_t* status) {
    TD_REQUIRE(raster && transform && xy && start && out && pos && status, "td_crown_zonal: null pointer");
    TD_REQUIRE(n >= 0 && n_xy >= 0, "td_crown_zonal: n = %d, n_xy = %lld, counts cannot be negative", n, (long long)n_xy);
    TD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols <= (int64_t)INT32_MAX,
               "td_crown_zonal: a %d x %d raster: both at least 1 and fewer than 2^31 pixels (the count is an int32)", rows, cols);
    for (int k = 0; k < 6; ++k)
        TD_REQUIRE(is_finite(transform[k]), "td_crown_zonal: transform[%d] is not finite", k);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(xy) % alignof(double) == 0, "td_crown_zonal: xy must be aligned to its doubles");
    const Affine t{transform[0], transform[1], transform[2], transform[3], transform[4], transform[5]};
    const float nan = std::numeric_limits<float>::quiet_NaN();
    constexpr int64_t RING_MAX = int64_t(1) << 30;      // a ring's vertex count is an int from here on
    std::vector<Pt> ring;
    std::vector<long long> inside;
    for (int q = 0; q < n; ++q) {
        float* o = out + 4 * (int64_t)q;
        int32_t* ps = pos + 3 * (int64_t)q;
        o[0] = o[1] = o[2] = o[3] = nan;
        ps[0] = ps[1] = ps[2] = -1;
        status[q] = 2;
        const int64_t s = start[q], e = start[q + 1];
        if (s < 0 || e < s || e > n_xy || e - s < 3 || e - s > RING_MAX) continue;
        const int m = (int)(e - s);
        const double inf = std::numeric_limits<double>::infinity();
        double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
        bool bad = false;
        ring.resize((size_t)m + 1);
        for (int k = 0; k <= m; ++k) {
            const double* p = xy + 2 * (s + (k == m ? 0 : k));
            bad |= !is_finite(p[0]) || !is_finite(p[1]);
            ring[k] = Pt{p[0], p[1]};
            x0 = p[0] < x0 ? p[0] : x0;
            y0 = p[1] < y0 ? p[1] : y0;
            x1 = p[0] > x1 ? p[0] : x1;
            y1 = p[1] > y1 ? p[1] : y1;
        }
        if (bad) continue;
        status[q] = 0;
        const Box B = pixel_box(t, x0, y0, x1, y1, rows, cols);
        float vmax = 0.f, vmin = 0.f;
        long long imax = -1, imin = -1;
        double sum = 0.0;
        inside.clear();
        for (int r = B.r0; r <= B.r1; ++r)
            for (int col = B.c0; col <= B.c1; ++col) {
                const Pt P = pixel_centre(t, r, col);
                if (!in_bounds(P, x0, y0, x1, y1) || tdgeom::point_in_query(ring.data(), m + 1, P) == 0) continue;
                const long long lin = (long long)r * cols + col;
                const float v = raster[lin];
                if (max_takes(v, lin, vmax, imax)) {
                    vmax = v;
                    imax = lin;
                }
                if (min_takes(v, lin, vmin, imin)) {
                    vmin = v;
                    imin = lin;
                }
                sum += (double)v;
                inside.push_back(lin);
            }
        const long long cnt = (long long)inside.size();
        if (cnt == 0) {
            o[0] = o[1] = o[2] = o[3] = -1.f;
            ps[0] = 0;
            continue;
        }
        const double mean = sum / (double)cnt;
        double sq = 0.0;
        for (const long long lin : inside) {
            const double dv = (double)raster[lin] - mean;
            sq += dv * dv;
        }
        o[0] = vmin;
        o[1] = vmax;
        o[2] = (float)mean;
        o[3] = (float)(sq / (double)cnt);
        ps[0] = (int32_t)cnt;
        ps[1] = (int32_t)(imax / cols);
        ps[2] = (int32_t)(imax % cols);
    }
    return TD_OK;
}
