// td_crown_labels (crownlabels_host.cpp, crown_zonal.h) in a program of its own, built with AddressSanitizer + UBSan
// (`make labels-check`): every buffer is a heap block of exactly the size the ABI states, so a read or write one element outside
// it ends the run.
//   1. crafted rings on a north-up raster whose centres are the half-integers, with pixel sets known by hand — a square with its
//      edges through centres, a triangle with vertices on centres, a diamond, a U, a bow-tie —, overlapping, with values that
//      include 0, 0x7FFFFFFF, 0x80000000 and 0xFFFFFFFF, over labels that hold a pattern already: every pixel against the unsigned
//      maximum restated over the known sets, in both orders of the rings;
//   2. rings off every side and corner of the raster, wholly outside (near and 1e300 away), a sliver between centres, on a 1 x 1
//      raster, rasters one row and one column wide, south-up, mirrored and rotated transforms: every pixel holds its old value or
//      a ring's, a ring around the raster fills it, rings outside change nothing;
//   3. refused crowns — 0, 1 and 2 vertices, NaN and infinite coordinates, a start below 0, an end past xy, a decreasing pair — get
//      status 2 and draw nothing while their neighbours are drawn;
//   4. malformed calls — null pointers, negative counts, an empty raster, 2^31 pixels, a non-finite transform, a misaligned xy —
//      are refused with TD_ERR_INVALID and a message, outputs untouched; n = 0 writes nothing.
// Exit status 0 and a final "ok" line on success; the first mismatch prints what differed and exits 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
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
    std::printf("labels_check: FAILED: %s (%ld, %.17g, %.17g)\n", what, a, b, c);
    std::exit(1);
}

struct RingSet {
    std::vector<double> xy;
    std::vector<int64_t> start{0};
    std::vector<uint32_t> value;
    void add(const std::vector<double>& ring, uint32_t v) {
        xy.insert(xy.end(), ring.begin(), ring.end());
        start.push_back((int64_t)xy.size() / 2);
        value.push_back(v);
    }
    int n() const { return (int)start.size() - 1; }
};

struct Grid {
    int rows, cols;
    double t[6];
};

Grid north_up(int rows, int cols) { return Grid{rows, cols, {1.0, 0.0, 0.0, 0.0, -1.0, (double)rows}}; }

std::vector<uint32_t> pattern(const Grid& G) {                       // every pixel its own small value, some 0
    std::vector<uint32_t> v((size_t)G.rows * G.cols);
    for (size_t k = 0; k < v.size(); ++k) v[k] = k % 5 == 0 ? 0u : (uint32_t)(100 + k);
    return v;
}

struct Result {
    std::vector<uint32_t> labels;
    std::vector<int32_t> status;
};

Result run(const Grid& G, const RingSet& S, const std::vector<uint32_t>& before, const std::vector<int64_t>* start_override = nullptr) {
    const std::vector<int64_t>& st = start_override ? *start_override : S.start;
    const int n = (int)st.size() - 1;
    auto xy = exact(S.xy.empty() ? std::vector<double>{0, 0} : S.xy);
    auto start = exact(st);
    auto value = exact(S.value.empty() ? std::vector<uint32_t>{0} : S.value);
    auto labels = exact(before);
    std::unique_ptr<int32_t[]> status(new int32_t[(size_t)std::max(n, 1)]);
    if (td_crown_labels(G.rows, G.cols, G.t, xy.get(), (int64_t)S.xy.size() / 2, start.get(), value.get(), n, labels.get(), status.get()) != TD_OK)
        fail(td_last_error());
    return {std::vector<uint32_t>(labels.get(), labels.get() + before.size()), std::vector<int32_t>(status.get(), status.get() + n)};
}

using Pred = std::function<bool(double, double)>;

void crafted() {
    const Grid G = north_up(16, 16);
    const std::vector<double> u = {1.2, 1.2, 10.8, 1.2, 10.8, 9.8, 7.8, 9.8, 7.8, 4.2, 4.2, 4.2, 4.2, 9.8, 1.2, 9.8};
    const std::vector<std::vector<double>> rings = {
        {2.5, 2.5, 6.5, 2.5, 6.5, 6.5, 2.5, 6.5},                        // edges through centres
        {1.5, 1.5, 4.5, 1.5, 1.5, 4.5},                                  // vertices on centres, hypotenuse through centres
        {5.5, 2.5, 8.5, 5.5, 5.5, 8.5, 2.5, 5.5},                        // a diamond
        u,
        {1.5, 1.5, 8.5, 8.5, 8.5, 1.5, 1.5, 8.5},                        // a bow-tie: even-odd
        {0.2, 0.2, 15.8, 0.2, 15.8, 15.8, 0.2, 15.8}};                   // the whole raster, value 0: changes nothing
    const std::vector<Pred> inside = {
        [](double x, double y) { return x >= 2.5 && x <= 6.5 && y >= 2.5 && y <= 6.5; },
        [](double x, double y) { return x >= 1.5 && y >= 1.5 && x + y <= 6.0; },
        [](double x, double y) { return std::fabs(x - 5.5) + std::fabs(y - 5.5) <= 3.0; },
        [](double x, double y) { return x > 1.2 && x < 10.8 && y > 1.2 && y < 9.8 && !(x > 4.2 && x < 7.8 && y > 4.2); },
        [](double x, double y) { return x >= 1.5 && x <= 8.5 && std::fabs(y - 5.0) <= std::fabs(x - 5.0); },
        [](double, double) { return true; }};
    const std::vector<uint32_t> values = {0x7FFFFFFFu, 0x80000000u, 7u, 0xFFFFFFFFu, 7u, 0u};
    const std::vector<uint32_t> before = pattern(G);
    for (int order = 0; order < 2; ++order) {
        RingSet S;
        for (size_t k = 0; k < rings.size(); ++k) {
            const size_t j = order ? rings.size() - 1 - k : k;
            S.add(rings[j], values[j]);
        }
        const Result res = run(G, S, before);
        for (int k = 0; k < S.n(); ++k)
            if (res.status[k] != 0) fail("a crafted ring is drawn", k, res.status[k]);
        for (int r = 0; r < G.rows; ++r)
            for (int c = 0; c < G.cols; ++c) {
                uint32_t want = before[(size_t)r * G.cols + c];
                for (size_t j = 0; j < rings.size(); ++j)
                    if (inside[j](c + 0.5, G.rows - (r + 0.5))) want = std::max(want, values[j]);
                if (res.labels[(size_t)r * G.cols + c] != want) fail("a crafted pixel", r * G.cols + c, res.labels[(size_t)r * G.cols + c], want);
            }
    }
}

void clipped_and_oriented() {
    const double th = 4.0 * M_PI / 180.0;
    const double transforms[6][6] = {{1, 0, 0, 0, -1, 9}, {0.5, 0, 1000, 0, 0.5, 2000}, {-0.5, 0, 1000, 0, -0.5, 2000}, {-0.5, 0, 1000, 0, 0.5, 2000},
                                     {0.5 * std::cos(th), 0.5 * std::sin(th), 1000, 0.5 * std::sin(th), -0.5 * std::cos(th), 2000},
                                     {0.2, 0, 412000.0, 0, -0.2, 5318060.0}};
    const int shapes[5][2] = {{9, 11}, {1, 1}, {1, 37}, {41, 1}, {3, 140}};
    for (const auto& tr : transforms)
        for (const auto& sh : shapes) {
            Grid G{sh[0], sh[1], {}};
            std::copy(tr, tr + 6, G.t);
            double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;       // the raster's corners in map coordinates
            for (int k = 0; k < 4; ++k) {
                const double u = (k & 1) ? sh[1] : 0, v = (k & 2) ? sh[0] : 0;
                const double x = tr[0] * u + tr[1] * v + tr[2], y = tr[3] * u + tr[4] * v + tr[5];
                x0 = std::min(x0, x), x1 = std::max(x1, x), y0 = std::min(y0, y), y1 = std::max(y1, y);
            }
            const double w = x1 - x0, h = y1 - y0, px = std::fabs(tr[0]);
            const bool rotated = tr[1] != 0;
            const std::vector<uint32_t> before = pattern(G);
            RingSet S;
            uint32_t next = 1000000u;
            const auto rect = [&](double a, double b, double c, double d) { S.add({a, b, c, b, c, d, a, d}, next++); };
            rect(x0 - w, y0 + 0.3 * h, x0 + 0.4 * w, y0 + 0.6 * h);               // off each side
            rect(x0 + 0.6 * w, y0 + 0.3 * h, x1 + w, y0 + 0.6 * h);
            rect(x0 + 0.3 * w, y0 - h, x0 + 0.6 * w, y0 + 0.4 * h);
            rect(x0 + 0.3 * w, y0 + 0.6 * h, x0 + 0.6 * w, y1 + h);
            rect(x0 - w, y0 - h, x0 + 0.3 * w, y0 + 0.3 * h);                     // off each corner
            rect(x0 + 0.7 * w, y0 + 0.7 * h, x1 + w, y1 + h);
            const Result part = run(G, S, before);
            for (size_t k = 0; k < before.size(); ++k)
                if (part.labels[k] != before[k] && (part.labels[k] < 1000000u || part.labels[k] >= next)) fail("a pixel holds its old value or a ring's", (long)k);
            RingSet O;                                                             // outside, far outside, a sliver between two centre columns
            O.add({x0 - 3 * w, y0, x0 - 2 * w, y0, x0 - 2 * w, y1, x0 - 3 * w, y1}, 0xFFFFFFFFu);
            O.add({1e300, 1e300, 1.5e300, 1e300, 1.5e300, 1.5e300, 1e300, 1.5e300}, 0xFFFFFFFFu);
            O.add({-1e300, -1e300, -1.5e300, -1e300, -1.5e300, -1.5e300, -1e300, -1.5e300}, 0xFFFFFFFFu);
            if (!rotated) O.add({x0 + 0.6 * px, y0 - h, x0 + 0.7 * px, y0 - h, x0 + 0.7 * px, y1 + h, x0 + 0.6 * px, y1 + h}, 0xFFFFFFFFu);
            const Result none = run(G, O, before);
            for (int k = 0; k < O.n(); ++k)
                if (none.status[k] != 0) fail("a ring outside the raster has status 0", k);
            if (none.labels != before) fail("rings outside the raster and between centres change nothing");
            if (!rotated) {
                RingSet A;
                A.add({x0 - w, y0 - h, x1 + w, y0 - h, x1 + w, y1 + h, x0 - w, y1 + h}, 0xFFFFFFFEu);
                const Result all = run(G, A, before);
                for (size_t k = 0; k < before.size(); ++k)
                    if (all.labels[k] != 0xFFFFFFFEu) fail("a ring around the raster fills it", (long)k);
            }
        }
    // the 1 x 1 raster, hit and missed
    const Grid one = north_up(1, 1);
    RingSet S;
    S.add({0.6, 0.2, 0.9, 0.2, 0.9, 0.8, 0.6, 0.8}, 9u);
    if (run(one, S, {4u}).labels[0] != 4u) fail("a ring beside the only centre draws nothing");
    S.add({0.5, 0.5, 3.0, 0.5, 3.0, 3.0, 0.5, 3.0}, 8u);                          // its corner ON the centre
    if (run(one, S, {4u}).labels[0] != 8u) fail("a ring whose corner is the only centre draws it");
    if (run(one, S, {0x80000000u}).labels[0] != 0x80000000u) fail("a larger value stays");
}

void refused() {
    const double nan = std::nan(""), inf = INFINITY;
    const Grid G = north_up(9, 9);
    RingSet S;
    S.add({1.2, 1.2, 4.8, 1.2, 4.8, 4.8, 1.2, 4.8}, 11u);      // 0: fine, 16 pixels
    S.add({}, 12u);                                            // 1: no vertices
    S.add({1, 1}, 13u);                                        // 2: one
    S.add({1, 1, 2, 2}, 14u);                                  // 3: two
    S.add({0, 0, nan, 0, 4, 4}, 15u);                          // 4
    S.add({0, 0, 4, -inf, 4, 4}, 16u);                         // 5
    S.add({3.2, 3.2, 6.8, 3.2, 6.8, 6.8, 3.2, 6.8}, 17u);      // 6: fine, the last ring of the buffer
    const std::vector<uint32_t> zeros(81, 0u);
    const Result res = run(G, S, zeros);
    long n11 = 0, n17 = 0;
    for (uint32_t v : res.labels) {
        if (v != 0u && v != 11u && v != 17u) fail("a refused crown drew", v);
        n11 += v == 11u, n17 += v == 17u;
    }
    if (n11 != 16 - 4 || n17 != 16) fail("the valid neighbours of refused crowns", n11, (double)n17);
    for (int k = 0; k < S.n(); ++k)
        if (res.status[k] != ((k == 0 || k == 6) ? 0 : 2)) fail("wrong status", k, res.status[k]);
    // starts that leave xy: that crown alone is refused
    const int64_t total = (int64_t)S.xy.size() / 2;
    RingSet T = S;
    T.value = {11u, 17u};
    const std::vector<std::vector<int64_t>> starts = {{-1, 4, total}, {0, 4, total + 1}, {0, total + 5, total}, {INT64_MIN, 4, total}, {0, 4, INT64_MAX}};
    const int bad[5] = {0, 1, 0, 0, 1};
    for (size_t v = 0; v < starts.size(); ++v) {
        const Result r2 = run(G, T, zeros, &starts[v]);
        if (r2.status[bad[v]] != 2) fail("a start outside xy is refused", (long)v, r2.status[bad[v]]);
        for (uint32_t l : r2.labels)
            if (l == (bad[v] == 0 ? 11u : 17u)) fail("a crown with a bad start drew", (long)v);
        if (v == 1 && (r2.status[0] != 0 || std::count(r2.labels.begin(), r2.labels.end(), 11u) != 16)) fail("the neighbour of a crown with a bad start is drawn", (long)v);
    }
}

void malformed() {
    const Grid G = north_up(4, 4);
    std::vector<double> xy = {0.25, 0.25, 3.75, 0.25, 0.25, 3.75, 9, 9};     // hypotenuse x + y = 4 through four centres: 10 pixels
    std::vector<int64_t> start = {0, 3};
    std::vector<uint32_t> value = {5u};
    std::vector<uint32_t> labels(16, 3u);
    int32_t status[1] = {9};
    const void* args[5] = {G.t, xy.data(), start.data(), value.data(), labels.data()};
    const auto call = [&](const void* const* a, int32_t* st, int rows, int cols, int64_t n_xy, int n) {
        return td_crown_labels(rows, cols, (const double*)a[0], (const double*)a[1], n_xy, (const int64_t*)a[2], (const uint32_t*)a[3], n,
                               (uint32_t*)const_cast<void*>(a[4]), st);
    };
    for (int k = 0; k < 6; ++k) {
        const void* a[5];
        std::copy(args, args + 5, a);
        if (k < 5) a[k] = nullptr;
        if (call(a, k == 5 ? nullptr : status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "null")) fail("a null pointer must be refused", k);
    }
    if (call(args, status, 4, 4, 3, -1) != TD_ERR_INVALID) fail("n < 0");
    if (call(args, status, 4, 4, -1, 1) != TD_ERR_INVALID) fail("n_xy < 0");
    if (call(args, status, 0, 4, 3, 1) != TD_ERR_INVALID || call(args, status, 4, 0, 3, 1) != TD_ERR_INVALID) fail("rows / cols < 1");
    if (call(args, status, -4, 4, 3, 1) != TD_ERR_INVALID) fail("rows < 0");
    if (call(args, status, 1 << 16, 1 << 15, 3, 1) != TD_ERR_INVALID) fail("2^31 pixels");
    {
        const void* a[5];
        std::copy(args, args + 5, a);
        a[1] = reinterpret_cast<const char*>(xy.data()) + 4;
        if (call(a, status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "aligned")) fail("a misaligned xy must be refused");
        for (int k = 0; k < 6; ++k) {
            double t[6];
            std::copy(G.t, G.t + 6, t);
            t[k] = k % 2 ? std::nan("") : INFINITY;
            std::copy(args, args + 5, a);
            a[0] = t;
            if (call(a, status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "finite")) fail("a non-finite transform must be refused", k);
        }
    }
    if (call(args, status, 4, 4, 3, 0) != TD_OK) fail("n = 0");
    for (uint32_t l : labels)
        if (l != 3u) fail("refused and empty calls must not write");
    if (status[0] != 9) fail("refused and empty calls must not write");
    if (call(args, status, 4, 4, 3, 1) != TD_OK || status[0] != 0 || std::count(labels.begin(), labels.end(), 5u) != 10) fail("the call itself is fine");
}

}  // namespace

int main() {
    crafted();
    clipped_and_oriented();
    refused();
    malformed();
    std::printf("labels_check: ok (crafted and overlapping rings, clipped and oriented rasters, refused crowns, malformed calls)\n");
    return 0;
}
