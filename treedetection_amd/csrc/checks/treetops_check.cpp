// td_treetops (treetops_host.cpp, treetops.h) in a program of its own, built with AddressSanitizer + UBSan (`make treetops-check`):
// every buffer is a heap block of exactly the size the ABI states, so a read or write one element outside it ends the run.
//   1. seeded random canopies (30 % zeros, some quantised to plateaus) on shapes from 1 x 1 to 70 x 131 — 1 x 9, 3 x 2 and 2 x 7 are
//      narrower than the radius, so an index is reflected more than once — with radius 0, 2, 4, 8 and 11 and windows 1, 3, 7, 15 and 33
//      (wider than the raster): marks, smoothed raster and counts against a restatement of the rule that walks the reflection step
//      by step and takes the window maximum over the k x k pixels directly;
//   2. the same with NaN, +inf and -inf pixels sown in (a NaN equals a NaN), floors of -inf and +inf, a raster of NaN only;
//   3. crafted spikes: alone, as equal twins inside and outside each other's window, exactly at the floor and one ulp above it;
//   4. optional outputs left out; malformed calls — null pointers, an empty raster, 2^31 pixels, an even window, a window below 1, a
//      negative radius, a NaN floor, NaN, infinite and asymmetric weights — refused with TD_ERR_INVALID and a message, outputs untouched.
// Exit status 0 and a final "ok" line on success; the first mismatch prints what differed and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../../include/treedet.h"

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {                // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

[[noreturn]] void fail(const char* what, long a = 0, double b = 0, double c = 0) {
    std::printf("treetops_check: FAILED: %s (%ld, %.17g, %.17g)\n", what, a, b, c);
    std::exit(1);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform() {                                                   // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

std::vector<double> gaussian(int r) {                                // a normalised symmetric table of radius r (any will do here)
    std::vector<double> w((size_t)2 * r + 1);
    const double sigma = r > 0 ? r / 4.0 : 1.0;
    double sum = 0;
    for (int i = -r; i <= r; ++i) sum += w[(size_t)(i + r)] = std::exp(-0.5 / (sigma * sigma) * i * i);
    for (int i = 0; i <= r; ++i) w[(size_t)(r + i)] = w[(size_t)(r - i)] = w[(size_t)(r - i)] / sum;
    return w;
}

int walk_reflect(long i, int n) {                                    // the reflection one step at a time: d c b a | a b c d | d c b a
    while (i < 0 || i >= n) i = i < 0 ? -1 - i : 2l * n - 1 - i;
    return (int)i;
}

struct Want {
    std::vector<float> smoothed;
    std::vector<uint8_t> marks;
    std::vector<int32_t> counts;
};

Want restate(const std::vector<float>& in, int rows, int cols, const std::vector<double>& w, int k, float floor) {
    const int r = ((int)w.size() - 1) / 2, h = k / 2;
    std::vector<float> a((size_t)rows * cols), s((size_t)rows * cols);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            double t = (double)in[(size_t)y * cols + x] * w[(size_t)r];
            for (int ii = -r; ii < 0; ++ii) {
                double pair = (double)in[(size_t)walk_reflect((long)y + ii, rows) * cols + x] + (double)in[(size_t)walk_reflect((long)y - ii, rows) * cols + x];
                double prod = pair * w[(size_t)(r + ii)];
                t = t + prod;
            }
            a[(size_t)y * cols + x] = (float)t;
        }
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            double t = (double)a[(size_t)y * cols + x] * w[(size_t)r];
            for (int ii = -r; ii < 0; ++ii) {
                double pair = (double)a[(size_t)y * cols + walk_reflect((long)x + ii, cols)] + (double)a[(size_t)y * cols + walk_reflect((long)x - ii, cols)];
                double prod = pair * w[(size_t)(r + ii)];
                t = t + prod;
            }
            s[(size_t)y * cols + x] = (float)t;
        }
    Want W{s, std::vector<uint8_t>((size_t)rows * cols), std::vector<int32_t>((size_t)rows, 0)};
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const float v = s[(size_t)y * cols + x];
            bool top = v > floor;                                    // (false for a NaN)
            for (int q = y - h; q <= y + h && top; ++q)
                for (int p = x - h; p <= x + h && top; ++p)
                    if (q >= 0 && q < rows && p >= 0 && p < cols && !std::isnan(s[(size_t)q * cols + p]) && !(v >= s[(size_t)q * cols + p])) top = false;
            W.marks[(size_t)y * cols + x] = top;
            W.counts[(size_t)y] += top;
        }
    return W;
}

bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, 4) == 0; }

long compare(const char* what, const std::vector<float>& in, int rows, int cols, const std::vector<double>& w, int k, float floor) {
    const size_t n = (size_t)rows * cols;
    auto raster = exact(in);
    auto weights = exact(w);
    std::unique_ptr<uint8_t[]> marks(new uint8_t[n]);
    std::unique_ptr<float[]> smoothed(new float[n]);
    std::unique_ptr<int32_t[]> counts(new int32_t[(size_t)rows]);
    const int r = ((int)w.size() - 1) / 2;
    if (td_treetops(raster.get(), rows, cols, weights.get(), r, k, floor, marks.get(), smoothed.get(), counts.get()) != TD_OK) fail(td_last_error());
    const Want W = restate(in, rows, cols, w, k, floor);
    long tops = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!same(smoothed[i], W.smoothed[i])) fail(what, (long)i, smoothed[i], W.smoothed[i]);
        if (marks[i] != W.marks[i]) fail(what, (long)i, marks[i], W.marks[i]);
        tops += marks[i];
    }
    for (int y = 0; y < rows; ++y)
        if (counts[(size_t)y] != W.counts[(size_t)y]) fail(what, y, counts[(size_t)y], W.counts[(size_t)y]);
    // the optional outputs left out: the same marks
    std::unique_ptr<uint8_t[]> alone(new uint8_t[n]);
    if (td_treetops(raster.get(), rows, cols, weights.get(), r, k, floor, alone.get(), nullptr, nullptr) != TD_OK) fail(td_last_error());
    if (std::memcmp(alone.get(), marks.get(), n) != 0) fail("marks without the optional outputs");
    return tops;
}

std::vector<float> canopy(int rows, int cols, bool plateaus, double nonfinite) {
    std::vector<float> v((size_t)rows * cols);
    const float special[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (float& x : v) {
        x = uniform() < 0.3 ? 0.0f : (float)(uniform() * 30.0);
        if (plateaus) x = std::round(x / 4.0f) * 4.0f;
        if (uniform() < nonfinite) x = special[(int)(uniform() * 3.0) % 3];
    }
    return v;
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 9}, {3, 2}, {2, 7}, {17, 5}, {5, 300}, {64, 64}, {70, 131}};
    const int radii[] = {0, 2, 4, 8, 11}, windows[] = {1, 3, 7, 15, 33};
    const float inf = std::numeric_limits<float>::infinity();
    long cases = 0, tops = 0;
    // 1, 2
    for (const auto& sh : shapes)
        for (int r : radii)
            for (int k : windows) {
                if ((long)sh[0] * sh[1] > 5000 && k > 15) continue;                  // (the restatement is k^2 per pixel)
                for (int kind = 0; kind < 3; ++kind) {
                    const std::vector<float> in = canopy(sh[0], sh[1], kind == 1, kind == 2 ? 0.02 : 0.0);
                    tops += compare(kind == 2 ? "non-finite canopy" : "canopy", in, sh[0], sh[1], gaussian(r), k, 3.0f);
                    ++cases;
                }
            }
    tops += compare("floor -inf", canopy(17, 5, true, 0.05), 17, 5, gaussian(2), 3, -inf);
    if (compare("floor +inf", canopy(17, 5, true, 0.05), 17, 5, gaussian(2), 3, inf) != 0) fail("a treetop above +inf");
    if (compare("NaN only", std::vector<float>(63, std::numeric_limits<float>::quiet_NaN()), 7, 9, gaussian(2), 7, 3.0f) != 0) fail("a NaN treetop");
    cases += 3;
    // 3
    {
        const int rows = 20, cols = 40;
        auto spikes = [&](std::initializer_list<int> at, float v) {
            std::vector<float> a((size_t)rows * cols, 0.0f);
            for (int i : at) a[(size_t)i] = v;
            return a;
        };
        for (int r : {0, 2}) {
            if (compare("one spike", spikes({0}, 10.0f), rows, cols, gaussian(r), 7, 3.0f) != 1) fail("one spike in the corner: one treetop");
            if (compare("one spike", spikes({rows * cols - 1}, 10.0f), rows, cols, gaussian(r), 7, 3.0f) != 1) fail("one spike in the last corner");
            if (compare("twins 3 apart", spikes({10 * cols + 10, 10 * cols + 13}, 10.0f), rows, cols, gaussian(r), 7, 3.0f) != 2) fail("equal twins in one window: both");
            if (compare("twins 4 apart", spikes({10 * cols + 10, 10 * cols + 14}, 10.0f), rows, cols, gaussian(r), 7, 3.0f) != 2) fail("twins apart: both");
            cases += 4;
        }
        if (compare("at the floor", spikes({45}, 3.0f), rows, cols, gaussian(0), 7, 3.0f) != 0) fail("a spike at the floor is no treetop");
        if (compare("an ulp above", spikes({45}, std::nextafter(3.0f, inf)), rows, cols, gaussian(0), 7, 3.0f) != 1) fail("a spike one ulp above the floor is one");
        cases += 2;
    }
    // 4
    {
        const std::vector<float> in(20, 5.0f);
        const std::vector<double> good = gaussian(2);
        auto raster = exact(in);
        auto call = [&](const float* ra, int rows, int cols, const std::vector<double>* w, int r, int k, float floor, bool with_marks) {
            std::unique_ptr<double[]> weights;
            if (w) weights = exact(*w);
            std::vector<uint8_t> before(20, 0x5A);
            auto marks = exact(before);
            std::vector<float> sb(20, -1.0f);
            auto smoothed = exact(sb);
            const td_status st = td_treetops(ra, rows, cols, weights.get(), r, k, floor, with_marks ? marks.get() : nullptr, smoothed.get(), nullptr);
            for (int i = 0; i < 20; ++i)
                if (marks[(size_t)i] != 0x5A || smoothed[(size_t)i] != -1.0f) fail("a refused call wrote an output", i);
            if (st != TD_ERR_INVALID) fail("a malformed call was not refused", st);
            if (std::strncmp(td_last_error(), "td_treetops:", 12) != 0) fail("a refusal without its message");
            ++cases;
        };
        const double nan = std::numeric_limits<double>::quiet_NaN(), dinf = std::numeric_limits<double>::infinity();
        const std::vector<double> w_nan{0.1, nan, 0.6, nan, 0.1}, w_inf{dinf, 0.2, 0.6, 0.2, dinf}, w_asym{0.1, 0.2, 0.4, 0.2, 0.11}, w_mid{0.1, 0.2, nan, 0.2, 0.1};
        call(nullptr, 4, 5, &good, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, nullptr, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, &good, 2, 7, 3.0f, false);
        call(raster.get(), 0, 5, &good, 2, 7, 3.0f, true);
        call(raster.get(), 4, -1, &good, 2, 7, 3.0f, true);
        call(raster.get(), 1 << 16, 1 << 15, &good, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, &good, 2, 6, 3.0f, true);
        call(raster.get(), 4, 5, &good, 2, 0, 3.0f, true);
        call(raster.get(), 4, 5, &good, 2, -7, 3.0f, true);
        call(raster.get(), 4, 5, &good, -1, 7, 3.0f, true);
        call(raster.get(), 4, 5, &good, 2, 7, std::numeric_limits<float>::quiet_NaN(), true);
        call(raster.get(), 4, 5, &w_nan, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, &w_inf, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, &w_asym, 2, 7, 3.0f, true);
        call(raster.get(), 4, 5, &w_mid, 2, 7, 3.0f, true);
    }
    std::printf("treetops_check: ok (%ld cases, %ld treetops)\n", cases, tops);
    return 0;
}
