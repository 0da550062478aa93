// The host twin of boxpairs_ab.hip: the same pair rule (include/treedet.h: comparisons only, nothing rounded) between two float64
// box sets, as a sweep instead of the kernel's all-against-all — the boxes of B with positive width and height sorted by x1, and
// for a row of A only the window of them whose x1 can satisfy the rule: x1_j < x2_i, and x1_j above x1_i minus the widest box of
// B. The window is a superset taken with outward-rounded bounds; the rule itself decides inside it, so the set is the kernel's
// for any input. Host code, one thread.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

struct Box {
    double x1, y1, x2, y2;
};

inline bool has_area(const Box& b) { return b.x2 > b.x1 && b.y2 > b.y1; }

}  // namespace

extern "C" td_status td_box_pairs_ab(const double* boxes_a, int n_a, const double* boxes_b, int n_b, int32_t* counts, int32_t* cols,
                                     int64_t cols_cap) {
    TD_REQUIRE(n_a >= 0 && n_b >= 0, "td_box_pairs_ab: n_a = %d, n_b = %d, a count is negative", n_a, n_b);
    TD_REQUIRE((boxes_a || n_a == 0) && (boxes_b || n_b == 0) && (counts || n_a == 0), "td_box_pairs_ab: null pointer");
    TD_REQUIRE(cols_cap >= 0, "td_box_pairs_ab: cols_cap = %lld is negative", (long long)cols_cap);
    const Box* a = reinterpret_cast<const Box*>(boxes_a);
    const Box* b = reinterpret_cast<const Box*>(boxes_b);
    std::vector<int32_t> order;
    order.reserve((size_t)n_b);
    double widest = 0.0;
    for (int j = 0; j < n_b; ++j)
        if (has_area(b[j])) {
            order.push_back(j);
            widest = std::max(widest, b[j].x2 - b[j].x1);       // (inf - (-inf) = inf; a finite difference is off by half an ulp at most)
        }
    const double inf = std::numeric_limits<double>::infinity();
    widest = std::nextafter(widest, inf);
    std::sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return b[p].x1 < b[q].x1 || (b[p].x1 == b[q].x1 && p < q); });
    std::vector<double> x1s(order.size());
    for (size_t k = 0; k < order.size(); ++k) x1s[k] = b[order[k]].x1;
    std::vector<int32_t> row;
    int64_t total = 0;
    for (int i = 0; i < n_a; ++i) {
        row.clear();
        const Box& r = a[i];
        if (has_area(r)) {
            double from = r.x1 - widest;                         // x1_j > x1_i - (x2_j - x1_j) >= x1_i - widest, one ulp of slack below
            from = std::isfinite(from) ? std::nextafter(from, -inf) : -inf;
            const size_t lo = std::lower_bound(x1s.begin(), x1s.end(), from) - x1s.begin();
            const size_t hi = std::lower_bound(x1s.begin(), x1s.end(), r.x2) - x1s.begin();      // x1_j < x2_i
            for (size_t k = lo; k < hi; ++k) {
                const Box& c = b[order[k]];
                if (r.x2 > c.x1 && c.x2 > r.x1 && r.y2 > c.y1 && c.y2 > r.y1) row.push_back(order[k]);
            }
            std::sort(row.begin(), row.end());
        }
        counts[i] = (int32_t)row.size();
        if (cols) {
            if (total + (int64_t)row.size() > cols_cap) {
                td_set_error("td_box_pairs_ab: cols holds %lld entries, row %d needs more", (long long)cols_cap, i);
                return TD_ERR_CAPACITY;
            }
            std::copy(row.begin(), row.end(), cols + total);
        }
        total += (int64_t)row.size();
    }
    return TD_OK;
}
