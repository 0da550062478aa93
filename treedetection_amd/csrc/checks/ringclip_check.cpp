// td_ring_pairs_area (ringiou_host.cpp, ring_clip.h) in a program of its own, built with AddressSanitizer + UBSan
// (`make ringclip-check`): every buffer is a heap block of exactly the size the ABI states, so a read or write one element
// outside it ends the run.
//   1. random star-shaped and convex rings of 3 - 70 vertices (small and UTM coordinates, some snapped to a 0.25 grid), random
//      pair lists over two ring sets: status 0, 0 <= inter <= min(area), the areas equal to a plain shoelace sum within 1e-9
//      relative, a ring with itself gives its own area, disjoint boxes give +0;
//   2. degenerate rings — every vertex the same point, all vertices on one line, repeated vertices — come out finite;
//   3. refused pairs — indices outside [0, n), rings of 0, 1 and 2 vertices, NaN and infinite coordinates — get status 2 and NaN
//      while their neighbours in the list are computed;
//   4. malformed calls — null pointers, negative counts — are refused with TD_ERR_INVALID and a message, outputs untouched;
//      n_pairs = 0 writes nothing.
// Exit status 0 and a final "ok" line on success; the first mismatch prints what differed and exits 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../../include/treedet.h"

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {                // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

[[noreturn]] void fail(const char* what, long a = 0, double b = 0, double c = 0) {
    std::printf("ringclip_check: FAILED: %s (%ld, %.17g, %.17g)\n", what, a, b, c);
    std::exit(1);
}

struct RingSet {
    std::vector<double> xy;
    std::vector<int64_t> start{0};
    void add(const std::vector<double>& ring) {
        xy.insert(xy.end(), ring.begin(), ring.end());
        start.push_back((int64_t)xy.size() / 2);
    }
    int n() const { return (int)start.size() - 1; }
};

std::vector<double> star(std::mt19937& rng, int m, double cx, double cy, bool convex, bool snap) {
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> ring;
    const double a = 2 + 4 * u(rng), b = 2 + 4 * u(rng), phase = 6.28 * u(rng);
    for (int k = 0; k < m; ++k) {
        const double ang = phase + (k + 0.15 + 0.7 * u(rng)) * (2 * M_PI / m), r = 2 + 5 * u(rng);
        double x = convex ? a * std::cos(ang) : r * std::cos(ang), y = convex ? b * std::sin(ang) : r * std::sin(ang);
        if (snap) x = std::round(4 * x) / 4, y = std::round(4 * y) / 4;
        ring.push_back(cx + x);
        ring.push_back(cy + y);
    }
    return ring;
}

double shoelace(const RingSet& s, int r) {
    const int64_t a = s.start[r], m = s.start[r + 1] - a;
    const double ox = s.xy[2 * a], oy = s.xy[2 * a + 1];
    double sum = 0;
    for (int64_t k = 0; k < m; ++k) {
        const int64_t k1 = (k + 1) % m;
        sum += (s.xy[2 * (a + k)] - ox) * (s.xy[2 * (a + k1) + 1] - oy) - (s.xy[2 * (a + k) + 1] - oy) * (s.xy[2 * (a + k1)] - ox);
    }
    return std::fabs(sum) / 2;
}

struct Result {
    std::vector<double> out;
    std::vector<int32_t> status;
};

Result run(const RingSet& A, const RingSet& B, const std::vector<int32_t>& pairs) {
    const int64_t k = (int64_t)pairs.size() / 2;
    auto xa = exact(A.xy.empty() ? std::vector<double>{0, 0} : A.xy), xb = exact(B.xy.empty() ? std::vector<double>{0, 0} : B.xy);
    auto sa = exact(A.start), sb = exact(B.start);
    auto pp = exact(pairs.empty() ? std::vector<int32_t>{0, 0} : pairs);
    std::unique_ptr<double[]> out(new double[(size_t)std::max<int64_t>(3 * k, 1)]);
    std::unique_ptr<int32_t[]> status(new int32_t[(size_t)std::max<int64_t>(k, 1)]);
    if (td_ring_pairs_area(xa.get(), sa.get(), A.n(), xb.get(), sb.get(), B.n(), pp.get(), k, out.get(), status.get()) != TD_OK)
        fail(td_last_error());
    return {std::vector<double>(out.get(), out.get() + 3 * k), std::vector<int32_t>(status.get(), status.get() + k)};
}

void random_case(std::mt19937& rng, double cx, double cy, bool snap) {
    std::uniform_real_distribution<double> u(0.0, 1.0);
    RingSet A, B;
    for (int r = 0; r < 9; ++r) {
        A.add(star(rng, 3 + (int)(rng() % 68), cx + 6 * u(rng), cy + 6 * u(rng), r % 2 == 0, snap));
        B.add(star(rng, 3 + (int)(rng() % 68), cx + 6 * u(rng), cy + 6 * u(rng), r % 3 == 0, snap));
    }
    B.add(star(rng, 5, cx + 500, cy + 500, true, snap));                 // far from everything
    std::vector<int32_t> pairs;
    for (int p = 0; p < 40; ++p) {
        pairs.push_back((int32_t)(rng() % A.n()));
        pairs.push_back((int32_t)(rng() % B.n()));
    }
    const Result res = run(A, B, pairs);
    for (size_t p = 0; p < res.status.size(); ++p) {
        const double inter = res.out[3 * p], ap = res.out[3 * p + 1], aq = res.out[3 * p + 2];
        if (res.status[p] != 0) fail("a valid pair was refused", (long)p);
        if (!(inter >= 0 && inter <= std::min(ap, aq)) || std::signbit(inter)) fail("inter outside [0, min(area)]", (long)p, inter, std::min(ap, aq));
        const double wp = shoelace(A, pairs[2 * p]), wq = shoelace(B, pairs[2 * p + 1]);
        if (std::fabs(ap - wp) > 1e-9 * wp || std::fabs(aq - wq) > 1e-9 * wq) fail("a ring area is off", (long)p, ap, wp);
        if (pairs[2 * p + 1] == B.n() - 1 && inter != 0.0) fail("disjoint boxes must give +0", (long)p, inter);
    }
    std::vector<int32_t> self;
    for (int r = 0; r < A.n(); ++r) self.push_back(r), self.push_back(r);
    const Result same = run(A, A, self);
    for (int r = 0; r < A.n(); ++r)
        if (same.status[r] != 0 || std::fabs(same.out[3 * r] - same.out[3 * r + 1]) > 1e-9 * same.out[3 * r + 1])
            fail("a ring with itself must give its own area", r, same.out[3 * r], same.out[3 * r + 1]);
}

void degenerate() {
    RingSet A;
    A.add({1, 1, 1, 1, 1, 1, 1, 1});                                     // one point four times
    A.add({0, 0, 1, 1, 2, 2, 3, 3});                                     // on one line
    A.add({0, 0, 4, 0, 4, 0, 4, 4, 0, 4, 0, 4});                         // a square with repeated vertices
    A.add({0, 0, 4, 0, 4, 4, 0, 4});
    std::vector<int32_t> pairs;
    for (int i = 0; i < A.n(); ++i)
        for (int j = 0; j < A.n(); ++j) pairs.push_back(i), pairs.push_back(j);
    const Result res = run(A, A, pairs);
    for (size_t p = 0; p < res.status.size(); ++p) {
        if (res.status[p] != 0) fail("a degenerate ring of >= 3 finite vertices is not refused", (long)p);
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(res.out[3 * p + c]) || res.out[3 * p + c] < 0) fail("a degenerate ring gave a non-finite or negative value", (long)p);
    }
    if (res.out[3 * (2 * 4 + 3)] != 16.0 || res.out[3 * (3 * 4 + 3)] != 16.0) fail("square with repeated vertices against the square", 0, res.out[3 * 11]);
    if (res.out[3 * (0 * 4 + 3)] != 0.0 || res.out[3 * (1 * 4 + 3)] != 0.0) fail("a point or a line has no area in common with a square");
}

void refused() {
    const double nan = std::nan(""), inf = INFINITY;
    RingSet A;
    A.add({0, 0, 4, 0, 4, 4, 0, 4});      // 0: fine
    A.add({});                            // 1: no vertices
    A.add({1, 1});                        // 2: one
    A.add({1, 1, 2, 2});                  // 3: two
    A.add({0, 0, nan, 0, 4, 4});          // 4
    A.add({0, 0, 4, -inf, 4, 4});         // 5
    A.add({1, 1, 3, 1, 2, 3});            // 6: fine, the last ring of the buffer
    const std::vector<int32_t> pairs = {0, 6, 7, 0, 0, 7, -1, 0, 0, -1, INT32_MAX, 0, INT32_MIN, 0, 1, 0, 0, 2, 3, 3, 4, 0, 0, 5, 6, 0};
    const Result res = run(A, A, pairs);
    const size_t k = res.status.size();
    for (size_t p = 0; p < k; ++p) {
        const bool good = p == 0 || p == k - 1;
        if (res.status[p] != (good ? 0 : 2)) fail("wrong status", (long)p, res.status[p]);
        for (int c = 0; c < 3; ++c)
            if (good == std::isnan(res.out[3 * p + c])) fail("NaN exactly for the refused pairs", (long)p);
    }
    if (std::fabs(res.out[0] - 2.0) > 1e-12 || std::fabs(res.out[3 * (k - 1)] - 2.0) > 1e-12) fail("the valid neighbours of refused pairs", 0, res.out[0]);
}

void malformed() {
    std::vector<double> xy = {0, 0, 1, 0, 0, 1};
    std::vector<int64_t> start = {0, 3};
    std::vector<int32_t> pairs = {0, 0};
    double out[3] = {7, 7, 7};
    int32_t status[1] = {9};
    const void* args[7] = {xy.data(), start.data(), xy.data(), start.data(), pairs.data(), out, status};
    for (int k = 0; k < 7; ++k) {
        const void* a[7];
        std::copy(args, args + 7, a);
        a[k] = nullptr;
        if (td_ring_pairs_area((const double*)a[0], (const int64_t*)a[1], 1, (const double*)a[2], (const int64_t*)a[3], 1, (const int32_t*)a[4], 1,
                               (double*)a[5], (int32_t*)a[6]) != TD_ERR_INVALID || !std::strstr(td_last_error(), "null"))
            fail("a null pointer must be refused", k);
    }
    if (td_ring_pairs_area(xy.data(), start.data(), 1, xy.data(), start.data(), 1, pairs.data(), -1, out, status) != TD_ERR_INVALID) fail("n_pairs < 0");
    if (td_ring_pairs_area(xy.data(), start.data(), -1, xy.data(), start.data(), 1, pairs.data(), 1, out, status) != TD_ERR_INVALID) fail("n_a < 0");
    if (td_ring_pairs_area(xy.data(), start.data(), 1, xy.data(), start.data(), 1, pairs.data(), 0, out, status) != TD_OK) fail("n_pairs = 0");
    if (out[0] != 7 || out[1] != 7 || out[2] != 7 || status[0] != 9) fail("refused and empty calls must not write");
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    int cases = 0;
    for (int trial = 0; trial < 12; ++trial, ++cases) random_case(rng, trial % 2 ? 4e5 : 0.0, trial % 2 ? 5e6 : 0.0, trial % 3 == 2);
    degenerate();
    refused();
    malformed();
    std::printf("ringclip_check: ok (%d random cases, degenerate rings, refused pairs, malformed calls)\n", cases);
    return 0;
}
