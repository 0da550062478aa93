// td_crown_pairs_greedy (pairgreedy.cpp) in a program of its own, built with AddressSanitizer + UBSan (`make pairgreedy-check`):
// every buffer is a heap block of exactly the size the ABI states, so a read or write one element outside it ends the run.
//   1. random symmetric masks with a random diagonal, confidences drawn from few float16 bit patterns (ties, both zeros,
//      subnormals, negatives, inf), rows stored shuffled → the removed flags of a dense restatement of the reference's group loop
//      (argmax over the mask row's ascending members with the row's own index appended);
//   2. malformed input — null pointers, n < 0, row_start not starting at 0 or decreasing, columns outside [0, n) — is refused
//      with TD_ERR_INVALID and a message, and `removed` is left untouched.
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

// float16 bit pattern → float by its definition (not the bit shuffling of pairgreedy.cpp)
float half_value(uint16_t h) {
    const int exp = (h >> 10) & 0x1f, man = h & 0x3ff;
    float v;
    if (exp == 0) v = std::ldexp((float)man, -24);
    else if (exp == 31) v = man ? NAN : INFINITY;
    else v = std::ldexp((float)(1024 + man), exp - 25);
    return (h & 0x8000) ? -v : v;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {                // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

[[noreturn]] void fail(const char* what, int a = 0, int b = 0) {
    std::printf("pairgreedy_check: %s (%d, %d)\n", what, a, b);
    std::exit(1);
}

void random_case(std::mt19937& rng, int n, double density, int trial) {
    const uint16_t palette[] = {0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0x3800, 0x3801, 0x3b33, 0x3c00, 0xb800, 0x7bff, 0x7c00};
    const int shades = 2 + (int)(rng() % (sizeof palette / sizeof *palette - 1));
    std::vector<uint16_t> conf(n);
    for (auto& c : conf) c = palette[rng() % shades];
    std::vector<uint8_t> mask((size_t)n * n, 0), diagonal(n);
    std::bernoulli_distribution edge(density);
    for (int i = 0; i < n; ++i) {
        diagonal[i] = rng() % 4 != 0;
        for (int j = i + 1; j < n; ++j) mask[(size_t)i * n + j] = mask[(size_t)j * n + i] = edge(rng);
    }
    const bool list_self = trial % 3 == 2;                          // the diagonal as entries of the rows instead of the flag array
    // the reference's loop on the dense mask
    std::vector<uint8_t> want(n, 0);
    for (int i = 0; i < n; ++i) {
        if (want[i]) continue;
        std::vector<int> members;
        for (int j = 0; j < n; ++j)
            if (j == i ? diagonal[i] : mask[(size_t)i * n + j]) members.push_back(j);
        members.push_back(i);
        int best = members[0];
        for (int j : members)
            if (half_value(conf[j]) > half_value(conf[best])) best = j;          // the first of the highest, as argmax
        for (int j : members)
            if (j != best) want[j] = 1;
    }
    // the same mask as shuffled sparse rows
    std::vector<int64_t> row_start(n + 1, 0);
    std::vector<int32_t> cols;
    for (int i = 0; i < n; ++i) {
        const size_t at = cols.size();
        for (int j = 0; j < n; ++j)
            if (j == i ? (list_self && diagonal[i]) : mask[(size_t)i * n + j]) cols.push_back(j);
        std::shuffle(cols.begin() + at, cols.end(), rng);
        row_start[i + 1] = (int64_t)cols.size();
    }
    auto rs = exact(row_start);
    auto cl = exact(cols);
    auto cf = exact(conf);
    auto dg = exact(diagonal);
    std::unique_ptr<uint8_t[]> removed(new uint8_t[n]);
    std::memset(removed.get(), 0xee, n);
    // with the diagonal listed in the rows the flag array may say "unset" everywhere: a row that lists itself still ties at its index
    if (list_self) std::memset(dg.get(), 0, n);
    if (td_crown_pairs_greedy(rs.get(), cols.empty() ? nullptr : cl.get(), cf.get(), dg.get(), n, removed.get()) != TD_OK)
        fail(td_last_error(), n, trial);
    for (int i = 0; i < n; ++i)
        if (removed[i] != want[i]) fail("removed flag differs from the dense loop's: n, row", n, i);
}

void expect_invalid(const char* what, const int64_t* rs, const int32_t* cl, const uint16_t* cf, int n, uint8_t* removed, int len) {
    std::memset(removed, 0xee, len);
    if (td_crown_pairs_greedy(rs, cl, cf, nullptr, n, removed) != TD_ERR_INVALID) fail(what, n, 0);
    if (!std::strstr(td_last_error(), "td_crown_pairs_greedy")) fail("no message for", n, 1);
    for (int i = 0; i < len; ++i)
        if (removed[i] != 0xee) fail("a refused call wrote to removed", n, i);
}

void malformed() {
    const std::vector<uint16_t> conf = {0x3800, 0x3900, 0x3a00};
    auto cf = exact(conf);
    std::unique_ptr<uint8_t[]> removed(new uint8_t[3]);
    struct Rows {
        const char* what;
        std::vector<int64_t> row_start;
        std::vector<int32_t> cols;
    };
    const Rows bad[] = {
        {"column n accepted", {0, 1, 1, 3}, {1, 0, 3}},
        {"negative column accepted", {0, 1, 2, 3}, {1, -1, 0}},
        {"INT32_MIN column accepted", {0, 1, 2, 3}, {1, INT32_MIN, 0}},
        {"decreasing row_start accepted", {0, 2, 1, 2}, {1, 2}},
        {"negative row_start accepted", {0, -1, 0, 0}, {1}},
        {"row_start[0] != 0 accepted", {1, 1, 1, 1}, {0}},
        {"huge row_start then a drop accepted", {0, INT64_MAX, 1, 1}, {1}},
    };
    for (const Rows& r : bad) {
        auto rs = exact(r.row_start);
        auto cl = exact(r.cols);
        expect_invalid(r.what, rs.get(), cl.get(), cf.get(), 3, removed.get(), 3);
    }
    const std::vector<int64_t> row_start = {0, 1, 2, 2};
    const std::vector<int32_t> cols = {1, 0};
    auto rs = exact(row_start);
    auto cl = exact(cols);
    expect_invalid("null row_start accepted", nullptr, cl.get(), cf.get(), 3, removed.get(), 3);
    expect_invalid("null cols with entries accepted", rs.get(), nullptr, cf.get(), 3, removed.get(), 3);
    expect_invalid("null conf accepted", rs.get(), cl.get(), nullptr, 3, removed.get(), 3);
    expect_invalid("n < 0 accepted", rs.get(), cl.get(), cf.get(), -1, removed.get(), 3);
    if (td_crown_pairs_greedy(rs.get(), cl.get(), cf.get(), nullptr, 3, nullptr) != TD_ERR_INVALID) fail("null removed accepted");
    // n = 0: one row_start entry, nothing else is read or written
    const std::vector<int64_t> zero = {0};
    auto rz = exact(zero);
    std::unique_ptr<uint8_t[]> none(new uint8_t[0]);
    std::unique_ptr<uint16_t[]> no_conf(new uint16_t[0]);
    if (td_crown_pairs_greedy(rz.get(), nullptr, no_conf.get(), nullptr, 0, none.get()) != TD_OK) fail("n = 0 refused");
    // the well-formed rows above: 0 ~ 1, confidences rising → 0 goes, 1 and 2 stay
    if (td_crown_pairs_greedy(rs.get(), cl.get(), cf.get(), nullptr, 3, removed.get()) != TD_OK) fail(td_last_error());
    if (removed[0] != 1 || removed[1] != 0 || removed[2] != 0) fail("the three-row example", removed[0], removed[1]);
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    int cases = 0;
    for (int n : {1, 2, 3, 7, 64, 301})
        for (double density : {0.0, 0.02, 0.3, 1.0})
            for (int trial = 0; trial < 6; ++trial, ++cases) random_case(rng, n, density, trial);
    malformed();
    std::printf("pairgreedy_check: ok (%d random cases, malformed rows refused)\n", cases);
    return 0;
}
