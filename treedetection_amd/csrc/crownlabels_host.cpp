// The host twin of td_crown_labels_dev (crownzonal.hip): crown outlines drawn into a uint32 label raster by unsigned maximum, the
// membership and the box from the same header (crown_zonal.h). It states the definition directly — point_in_query over ALL edges of
// the ring for every pixel of the box — and has no vertex cap: it serves the crowns the kernel marks status 1, the host path of
// crown_label_raster (device=None) and the CPU tests. The maximum does not depend on the order of the crowns, so the raster equals
// the device's bit for bit. Nothing is cleared: the caller's labels are composited over. Host code.
#include "common.h"
#include "crown_zonal.h"

#include <limits>
#include <vector>

using namespace tdzonal;

extern "C" td_status td_crown_labels(int rows, int cols, const double* transform, const double* xy, int64_t n_xy, const int64_t* start,
                                     const uint32_t* value, int n, uint32_t* labels, int32_t* status) {
    TD_REQUIRE(transform && xy && start && value && labels && status, "td_crown_labels: null pointer");
    TD_REQUIRE(n >= 0 && n_xy >= 0, "td_crown_labels: n = %d, n_xy = %lld, counts cannot be negative", n, (long long)n_xy);
    TD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols <= (int64_t)INT32_MAX,
               "td_crown_labels: a %d x %d raster: both at least 1 and fewer than 2^31 pixels", rows, cols);
    for (int k = 0; k < 6; ++k)
        TD_REQUIRE(is_finite(transform[k]), "td_crown_labels: transform[%d] is not finite", k);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(xy) % alignof(double) == 0, "td_crown_labels: xy must be aligned to its doubles");
    const Affine t{transform[0], transform[1], transform[2], transform[3], transform[4], transform[5]};
    constexpr int64_t RING_MAX = int64_t(1) << 30;      // a ring's vertex count is an int from here on
    std::vector<Pt> ring;
    for (int q = 0; q < n; ++q) {
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
        const uint32_t v = value[q];
        if (v == 0u) continue;                          // the maximum with 0 changes nothing
        const Box B = pixel_box(t, x0, y0, x1, y1, rows, cols);
        for (int r = B.r0; r <= B.r1; ++r)
            for (int col = B.c0; col <= B.c1; ++col) {
                const Pt P = pixel_centre(t, r, col);
                if (!in_bounds(P, x0, y0, x1, y1) || tdgeom::point_in_query(ring.data(), m + 1, P) == 0) continue;
                uint32_t* l = labels + ((int64_t)r * cols + col);
                *l = v > *l ? v : *l;
            }
    }
    return TD_OK;
}
