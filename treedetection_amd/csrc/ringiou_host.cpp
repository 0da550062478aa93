// The host twin of td_ring_pairs_area_dev (ringiou.hip): the same arithmetic from the same header (ring_clip.h), the wave's 64
// lanes emulated, so that the two agree bit for bit. It has no vertex cap: it serves the pairs the kernel marks status 1, the
// host path of clean_crowns (device=None) and the CPU tests. Host code.
#include "common.h"
#include "ring_clip.h"

#include <limits>
#include <vector>

extern "C" td_status td_ring_pairs_area(const double* xy_a, const int64_t* start_a, int n_a, const double* xy_b, const int64_t* start_b,
                                        int n_b, const int32_t* pairs, int64_t n_pairs, double* out, int32_t* status) {
    TD_REQUIRE(xy_a && start_a && xy_b && start_b && pairs && out && status, "td_ring_pairs_area: null pointer");
    TD_REQUIRE(n_a >= 0 && n_b >= 0, "td_ring_pairs_area: n_a = %d, n_b = %d, ring counts cannot be negative", n_a, n_b);
    TD_REQUIRE(n_pairs >= 0, "td_ring_pairs_area: n_pairs = %lld is negative", (long long)n_pairs);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    constexpr int64_t RING_MAX = int64_t(1) << 30;      // a ring's vertex count is an int from here on
    std::vector<double> scratch;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
        double* o = out + 3 * p;
        o[0] = o[1] = o[2] = nan;
        status[p] = 2;
        if (ia < 0 || ia >= n_a || ib < 0 || ib >= n_b) continue;
        const int64_t a0 = start_a[ia], b0 = start_b[ib];
        const int64_t ma = start_a[ia + 1] - a0, mb = start_b[ib + 1] - b0;
        if (a0 < 0 || b0 < 0 || ma < 3 || mb < 3 || ma > RING_MAX || mb > RING_MAX) continue;
        const double* xa = xy_a + 2 * a0;
        const double* xb = xy_b + 2 * b0;
        bool bad = false;
        for (int64_t k = 0; k < 2 * ma; ++k) bad |= !rc_finite(xa[k]);
        for (int64_t k = 0; k < 2 * mb; ++k) bad |= !rc_finite(xb[k]);
        if (bad) continue;
        if (scratch.size() < (size_t)(2 * (ma + mb))) scratch.resize((size_t)(2 * (ma + mb)));
        double* px = scratch.data();
        rc_pair_host(xa, (int)ma, xb, (int)mb, px, px + ma, px + 2 * ma, px + 2 * ma + mb, o);
        status[p] = 0;
    }
    return TD_OK;
}
