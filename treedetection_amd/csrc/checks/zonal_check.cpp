// td_crown_zonal (crownzonal_host.cpp, crown_zonal.h) in a program of its own, built with AddressSanitizer + UBSan
// (`make zonal-check`): every buffer is a heap block of exactly the size the ABI states, so a read or write one element outside
// it ends the run.
//   1. crafted rings on a north-up raster whose centres are the half-integers, with pixel sets known by hand: a square with its
//      edges through centres, a triangle with vertices on centres, a diamond with vertices on a centre row, a U whose notch holds the
//      raster's largest value, the U reversed, a bow-tie; count, position of the maximum, minimum and maximum against a plain
//      restatement over the known set;
//   2. rings off every side and corner of the raster, wholly outside (near and 1e300 away), a sliver between centres, a 1 x 1
//      raster, rasters one row and one column wide, south-up, mirrored and rotated transforms: counts between 0 and the raster's
//      size, positions inside the raster, the empty rows all -1;
//   3. random star rings of 3 - 700 vertices at small and UTM coordinates: count equal to a crossing count written out here with
//      long double determinants wherever that count is clear of every edge by 1e-6;
//   4. refused crowns — 0, 1 and 2 vertices, NaN and infinite coordinates, a start below 0, an end past xy, a decreasing pair — get
//      status 2, NaN and -1 while their neighbours are computed;
//   5. malformed calls — null pointers, negative counts, an empty raster, a non-finite transform, a misaligned xy — are refused with
//      TD_ERR_INVALID and a message, outputs untouched; n = 0 writes nothing.
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
    std::printf("zonal_check: FAILED: %s (%ld, %.17g, %.17g)\n", what, a, b, c);
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

struct Raster {
    int rows, cols;
    std::vector<float> v;
    double t[6];
};

Raster north_up(int rows, int cols, unsigned seed) {                 // x = col + 0.5, y = rows - (row + 0.5); distinct values in (0.25, 1)
    Raster R{rows, cols, std::vector<float>((size_t)rows * cols), {1.0, 0.0, 0.0, 0.0, -1.0, (double)rows}};
    std::vector<int> perm(R.v.size());
    for (size_t k = 0; k < perm.size(); ++k) perm[k] = (int)k;
    std::mt19937 rng(seed);
    std::shuffle(perm.begin(), perm.end(), rng);
    for (size_t k = 0; k < perm.size(); ++k) R.v[k] = (float)(0.25 + 0.75 * (perm[k] + 0.5) / (double)perm.size());
    return R;
}

struct Result {
    std::vector<float> out;
    std::vector<int32_t> pos, status;
};

Result run(const Raster& R, const RingSet& S, const std::vector<int64_t>* start_override = nullptr) {
    const std::vector<int64_t>& st = start_override ? *start_override : S.start;
    const int n = (int)st.size() - 1;
    auto raster = exact(R.v);
    auto xy = exact(S.xy.empty() ? std::vector<double>{0, 0} : S.xy);
    auto start = exact(st);
    std::unique_ptr<float[]> out(new float[(size_t)std::max(4 * n, 1)]);
    std::unique_ptr<int32_t[]> pos(new int32_t[(size_t)std::max(3 * n, 1)]), status(new int32_t[(size_t)std::max(n, 1)]);
    if (td_crown_zonal(raster.get(), R.rows, R.cols, R.t, xy.get(), (int64_t)S.xy.size() / 2, start.get(), n, out.get(), pos.get(), status.get()) !=
        TD_OK)
        fail(td_last_error());
    return {std::vector<float>(out.get(), out.get() + 4 * n), std::vector<int32_t>(pos.get(), pos.get() + 3 * n),
            std::vector<int32_t>(status.get(), status.get() + n)};
}

// crown k of res against the pixel set `in` (row-major (row, col) pairs), values distinct and finite
void against_set(const Raster& R, const Result& res, int k, const std::vector<std::pair<int, int>>& in, const char* what) {
    if (res.status[k] != 0) fail(what, k, res.status[k]);
    if (res.pos[3 * k] != (int32_t)in.size()) fail(what, k, res.pos[3 * k], (double)in.size());
    if (in.empty()) {
        for (int c = 0; c < 4; ++c)
            if (res.out[4 * k + c] != -1.f) fail("an empty crown has -1 everywhere", k);
        if (res.pos[3 * k + 1] != -1 || res.pos[3 * k + 2] != -1) fail("an empty crown has position -1", k);
        return;
    }
    float lo = INFINITY, hi = -INFINITY;
    int hr = -1, hc = -1;
    double sum = 0;
    for (const auto& p : in) {
        const float v = R.v[(size_t)p.first * R.cols + p.second];
        lo = std::min(lo, v);
        if (v > hi) hi = v, hr = p.first, hc = p.second;
        sum += v;
    }
    if (res.out[4 * k] != lo || res.out[4 * k + 1] != hi) fail("minimum / maximum", k, res.out[4 * k], res.out[4 * k + 1]);
    if (res.pos[3 * k + 1] != hr || res.pos[3 * k + 2] != hc) fail("position of the maximum", k, res.pos[3 * k + 1], res.pos[3 * k + 2]);
    const double mean = sum / (double)in.size();
    if (std::fabs(res.out[4 * k + 2] - mean) > 1e-6 * mean) fail("mean", k, res.out[4 * k + 2], mean);
    double sq = 0;
    for (const auto& p : in) sq += (R.v[(size_t)p.first * R.cols + p.second] - mean) * (R.v[(size_t)p.first * R.cols + p.second] - mean);
    if (std::fabs(res.out[4 * k + 3] - sq / (double)in.size()) > 1e-5 * (sq / (double)in.size()) + 1e-12) fail("variance", k, res.out[4 * k + 3]);
}

// the pixels of a north-up raster whose centre (x, y) satisfies pred, row-major
template <class Pred>
std::vector<std::pair<int, int>> pixels(const Raster& R, Pred pred) {
    std::vector<std::pair<int, int>> in;
    for (int r = 0; r < R.rows; ++r)
        for (int c = 0; c < R.cols; ++c)
            if (pred(c + 0.5, R.rows - (r + 0.5))) in.push_back({r, c});
    return in;
}

void crafted() {
    Raster R = north_up(16, 16, 7);
    const std::vector<double> u = {1.2, 1.2, 10.8, 1.2, 10.8, 9.8, 7.8, 9.8, 7.8, 4.2, 4.2, 4.2, 4.2, 9.8, 1.2, 9.8};
    std::vector<double> u_rev;
    for (int k = (int)u.size() / 2 - 1; k >= 0; --k) u_rev.push_back(u[2 * k]), u_rev.push_back(u[2 * k + 1]);
    R.v[(size_t)(16 - 7) * 16 + 5] = 9.f;                               // in the U's notch (x 5.5, y 6.5): the raster's largest value
    RingSet S;
    S.add({2.5, 2.5, 6.5, 2.5, 6.5, 6.5, 2.5, 6.5});                     // 0: edges through centres
    S.add({1.5, 1.5, 4.5, 1.5, 1.5, 4.5});                               // 1: vertices on centres, hypotenuse through centres
    S.add({5.5, 2.5, 8.5, 5.5, 5.5, 8.5, 2.5, 5.5});                     // 2: a diamond, left and right vertices on a centre row
    S.add(u);                                                            // 3
    S.add(u_rev);                                                        // 4
    S.add({1.5, 1.5, 8.5, 8.5, 8.5, 1.5, 1.5, 8.5});                     // 5: a bow-tie: even-odd, the crossing (5, 5) on no centre
    const Result res = run(R, S);
    against_set(R, res, 0, pixels(R, [](double x, double y) { return x >= 2.5 && x <= 6.5 && y >= 2.5 && y <= 6.5; }), "square");
    against_set(R, res, 1, pixels(R, [](double x, double y) { return x >= 1.5 && y >= 1.5 && x + y <= 6.0; }), "triangle");
    against_set(R, res, 2, pixels(R, [](double x, double y) { return std::fabs(x - 5.5) + std::fabs(y - 5.5) <= 3.0; }), "diamond");
    const auto in_u = [](double x, double y) { return x > 1.2 && x < 10.8 && y > 1.2 && y < 9.8 && !(x > 4.2 && x < 7.8 && y > 4.2); };
    against_set(R, res, 3, pixels(R, in_u), "U");
    against_set(R, res, 4, pixels(R, in_u), "U reversed");
    if (res.out[4 * 3 + 1] >= 9.f) fail("the notch of the U is outside it");
    against_set(R, res, 5, pixels(R, [](double x, double y) {          // left and right triangles of the bow-tie, boundary included
        return x >= 1.5 && x <= 8.5 && std::fabs(y - 5.0) <= std::fabs(x - 5.0); }), "bow-tie");
}

void clipped_and_oriented() {
    const double th = 4.0 * M_PI / 180.0;
    const double transforms[6][6] = {{1, 0, 0, 0, -1, 9}, {0.5, 0, 1000, 0, 0.5, 2000}, {-0.5, 0, 1000, 0, -0.5, 2000}, {-0.5, 0, 1000, 0, 0.5, 2000},
                                     {0.5 * std::cos(th), 0.5 * std::sin(th), 1000, 0.5 * std::sin(th), -0.5 * std::cos(th), 2000},
                                     {0.2, 0, 412000.0, 0, -0.2, 5318060.0}};
    const int shapes[5][2] = {{9, 11}, {1, 1}, {1, 37}, {41, 1}, {3, 140}};
    for (const auto& tr : transforms)
        for (const auto& sh : shapes) {
            Raster R = north_up(sh[0], sh[1], 11);
            std::copy(tr, tr + 6, R.t);
            // the raster's corners in map coordinates → rectangles around, across and beside it
            double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
            for (int k = 0; k < 4; ++k) {
                const double u = (k & 1) ? sh[1] : 0, v = (k & 2) ? sh[0] : 0;
                const double x = tr[0] * u + tr[1] * v + tr[2], y = tr[3] * u + tr[4] * v + tr[5];
                x0 = std::min(x0, x), x1 = std::max(x1, x), y0 = std::min(y0, y), y1 = std::max(y1, y);
            }
            const double w = x1 - x0, h = y1 - y0, px = std::fabs(tr[0]);
            RingSet S;
            const auto rect = [&](double a, double b, double c, double d) { S.add({a, b, c, b, c, d, a, d}); };
            rect(x0 - w, y0 - h, x1 + w, y1 + h);                                 // 0: everything
            rect(x0 - w, y0 + 0.3 * h, x0 + 0.4 * w, y0 + 0.6 * h);               // off each side
            rect(x0 + 0.6 * w, y0 + 0.3 * h, x1 + w, y0 + 0.6 * h);
            rect(x0 + 0.3 * w, y0 - h, x0 + 0.6 * w, y0 + 0.4 * h);
            rect(x0 + 0.3 * w, y0 + 0.6 * h, x0 + 0.6 * w, y1 + h);
            rect(x0 - w, y0 - h, x0 + 0.3 * w, y0 + 0.3 * h);                     // off each corner
            rect(x0 + 0.7 * w, y0 + 0.7 * h, x1 + w, y1 + h);
            rect(x0 - 3 * w, y0, x0 - 2 * w, y1);                                 // 7: outside
            rect(1e300, 1e300, 1.5e300, 1.5e300);                                 // 8: far outside
            rect(x0 + 0.5 * px + 0.1 * px, y0 - h, x0 + 0.5 * px + 0.2 * px, y1 + h);   // 9: a sliver (axis-aligned: between two centre columns)
            const Result res = run(R, S);
            const bool rotated = tr[1] != 0;
            if (!rotated && res.pos[0] != sh[0] * sh[1]) fail("a ring around the raster holds every pixel", res.pos[0], sh[0] * sh[1]);
            for (int k = 0; k < S.n(); ++k) {
                if (res.status[k] != 0) fail("a clipped ring is computed", k);
                const int cnt = res.pos[3 * k];
                if (cnt < 0 || cnt > sh[0] * sh[1]) fail("count outside [0, pixels]", k, cnt);
                if (cnt == 0 && (res.pos[3 * k + 1] != -1 || res.out[4 * k] != -1.f)) fail("an empty crown is all -1", k);
                if (cnt > 0 && (res.pos[3 * k + 1] < 0 || res.pos[3 * k + 1] >= sh[0] || res.pos[3 * k + 2] < 0 || res.pos[3 * k + 2] >= sh[1]))
                    fail("the maximum lies inside the raster", k, res.pos[3 * k + 1], res.pos[3 * k + 2]);
            }
            if (res.pos[3 * 7] != 0 || res.pos[3 * 8] != 0) fail("rings outside the raster hold nothing");
            if (!rotated && res.pos[3 * 9] != 0) fail("a sliver between centre columns holds nothing", res.pos[3 * 9]);
        }
}

void random_stars() {
    std::mt19937 rng(20260114);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    long checked = 0;
    for (int trial = 0; trial < 10; ++trial) {
        Raster R = north_up(40, 48, 100 + trial);
        const bool utm = trial % 2;
        const double px = utm ? 0.2 : 1.0;
        const double tr[6] = {px, 0, utm ? 412000.0 : 0.0, 0, -px, utm ? 5318060.0 : 40.0};
        std::copy(tr, tr + 6, R.t);
        RingSet S;
        for (int k = 0; k < 12; ++k) {
            const int m = k == 11 ? 700 : 3 + (int)(rng() % 60);
            const double cx = tr[2] + px * (4 + 40 * u(rng)), cy = tr[5] - px * (4 + 32 * u(rng));
            std::vector<double> ring;
            for (int j = 0; j < m; ++j) {
                const double ang = (j + 0.1 + 0.8 * u(rng)) * (2 * M_PI / m), r = px * (1 + 8 * u(rng));
                ring.push_back(cx + r * std::cos(ang));
                ring.push_back(cy + r * std::sin(ang));
            }
            S.add(ring);
        }
        const Result res = run(R, S);
        for (int k = 0; k < S.n(); ++k) {
            if (res.status[k] != 0) fail("a star ring is computed", k);
            const int64_t a = S.start[k], m = S.start[k + 1] - a;
            int count = 0;
            bool clear = true;
            for (int r = 0; r < R.rows && clear; ++r)
                for (int c = 0; c < R.cols && clear; ++c) {
                    const long double x = (long double)tr[0] * (c + 0.5L) + tr[2], y = (long double)tr[4] * (r + 0.5L) + tr[5];
                    bool odd = false;
                    for (int64_t j = 0; j < m; ++j) {
                        const long double ax = S.xy[2 * (a + j)], ay = S.xy[2 * (a + j) + 1], bx = S.xy[2 * (a + (j + 1) % m)],
                                          by = S.xy[2 * (a + (j + 1) % m) + 1];
                        const long double det = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
                        const long double len = std::sqrt((double)((bx - ax) * (bx - ax) + (by - ay) * (by - ay)));
                        if (std::fabs((double)(y - ay)) < 1e-6 * px || std::fabs((double)(y - by)) < 1e-6 * px ||
                            (std::fabs((double)det) < 1e-6 * px * (double)len && y >= std::min(ay, by) && y <= std::max(ay, by)))
                            clear = false;                               // too close to call here: this ring is left to the exact tests
                        if ((ay <= y) != (by <= y) && ((ay <= y) ? det > 0 : det < 0)) odd = !odd;
                    }
                    count += odd;
                }
            if (!clear) continue;
            ++checked;
            if (res.pos[3 * k] != count) fail("count of a star ring", k, res.pos[3 * k], count);
        }
    }
    if (checked < 60) fail("too few star rings were clear of every centre", checked);
}

void refused() {
    const double nan = std::nan(""), inf = INFINITY;
    Raster R = north_up(9, 9, 3);
    RingSet S;
    S.add({1.2, 1.2, 4.8, 1.2, 4.8, 4.8, 1.2, 4.8});      // 0: fine, 16 pixels
    S.add({});                                            // 1: no vertices
    S.add({1, 1});                                        // 2: one
    S.add({1, 1, 2, 2});                                  // 3: two
    S.add({0, 0, nan, 0, 4, 4});                          // 4
    S.add({0, 0, 4, -inf, 4, 4});                         // 5
    S.add({3.2, 3.2, 6.8, 3.2, 6.8, 6.8, 3.2, 6.8});      // 6: fine, the last ring of the buffer
    const Result res = run(R, S);
    for (int k = 0; k < S.n(); ++k) {
        const bool good = k == 0 || k == 6;
        if (res.status[k] != (good ? 0 : 2)) fail("wrong status", k, res.status[k]);
        for (int c = 0; c < 4; ++c)
            if (good == std::isnan(res.out[4 * k + c])) fail("NaN exactly for the refused crowns", k);
        if (!good && (res.pos[3 * k] != -1 || res.pos[3 * k + 1] != -1 || res.pos[3 * k + 2] != -1)) fail("-1 for the refused crowns", k);
        if (good && res.pos[3 * k] != 16) fail("the valid neighbours of refused crowns", k, res.pos[3 * k]);
    }
    // starts that leave xy: that crown alone is refused
    const int64_t total = (int64_t)S.xy.size() / 2;
    const std::vector<std::vector<int64_t>> starts = {{-1, 4, total}, {0, 4, total + 1}, {0, total + 5, total}, {INT64_MIN, 4, total}, {0, 4, INT64_MAX}};
    const int bad[5] = {0, 1, 0, 0, 1};
    for (size_t v = 0; v < starts.size(); ++v) {
        const Result r2 = run(R, S, &starts[v]);
        if (r2.status[bad[v]] != 2 || !std::isnan(r2.out[4 * bad[v]])) fail("a start outside xy is refused", (long)v, r2.status[bad[v]]);
        if (v == 1 && (r2.status[0] != 0 || r2.pos[0] != 16)) fail("the neighbour of a crown with a bad start is computed", (long)v);
    }
}

void malformed() {
    Raster R = north_up(4, 4, 5);
    std::vector<double> xy = {0.25, 0.25, 3.75, 0.25, 0.25, 3.75, 9, 9};     // hypotenuse x + y = 4 through four centres: 10 pixels
    std::vector<int64_t> start = {0, 3};
    float out[4] = {7, 7, 7, 7};
    int32_t pos[3] = {9, 9, 9}, status[1] = {9};
    const void* args[6] = {R.v.data(), R.t, xy.data(), start.data(), out, pos};
    const auto call = [&](const void* const* a, int32_t* st, int rows, int cols, int64_t n_xy, int n) {
        return td_crown_zonal((const float*)a[0], rows, cols, (const double*)a[1], (const double*)a[2], n_xy, (const int64_t*)a[3], n, (float*)a[4],
                              (int32_t*)a[5], st);
    };
    for (int k = 0; k < 7; ++k) {
        const void* a[6];
        std::copy(args, args + 6, a);
        if (k < 6) a[k] = nullptr;
        if (call(a, k == 6 ? nullptr : status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "null")) fail("a null pointer must be refused", k);
    }
    if (call(args, status, 4, 4, 3, -1) != TD_ERR_INVALID) fail("n < 0");
    if (call(args, status, 4, 4, -1, 1) != TD_ERR_INVALID) fail("n_xy < 0");
    if (call(args, status, 0, 4, 3, 1) != TD_ERR_INVALID || call(args, status, 4, 0, 3, 1) != TD_ERR_INVALID) fail("rows / cols < 1");
    if (call(args, status, 1 << 16, 1 << 15, 3, 1) != TD_ERR_INVALID) fail("2^31 pixels");
    {
        const void* a[6];
        std::copy(args, args + 6, a);
        a[2] = reinterpret_cast<const char*>(xy.data()) + 4;
        if (call(a, status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "aligned")) fail("a misaligned xy must be refused");
        double t[6];
        std::copy(R.t, R.t + 6, t);
        t[4] = std::nan("");
        std::copy(args, args + 6, a);
        a[1] = t;
        if (call(a, status, 4, 4, 3, 1) != TD_ERR_INVALID || !std::strstr(td_last_error(), "finite")) fail("a non-finite transform must be refused");
    }
    if (call(args, status, 4, 4, 3, 0) != TD_OK) fail("n = 0");
    for (int c = 0; c < 4; ++c)
        if (out[c] != 7) fail("refused and empty calls must not write");
    if (pos[0] != 9 || pos[1] != 9 || pos[2] != 9 || status[0] != 9) fail("refused and empty calls must not write");
    if (call(args, status, 4, 4, 3, 1) != TD_OK || status[0] != 0 || pos[0] != 10) fail("the call itself is fine", pos[0]);
}

}  // namespace

int main() {
    crafted();
    clipped_and_oriented();
    random_stars();
    refused();
    malformed();
    std::printf("zonal_check: ok (crafted rings, clipped and oriented rasters, random stars, refused crowns, malformed calls)\n");
    return 0;
}
