// td_box_pairs_ab (boxpairs_ab_host.cpp) and td_match_greedy (matchgreedy.cpp) in a program of their own, built with
// AddressSanitizer + UBSan (`make evaluation-check`): every buffer is a heap block of exactly the size the ABI states, so a read
// or write one element outside it ends the run.
//   1. random box sets — jittered grids, coordinates from a small lattice (touching and identical boxes), zero-width and inverted
//      boxes, NaN and infinite coordinates, an empty side — against the pair rule written as min / max over all n_a x n_b pairs;
//      rows ascending; the capacity check; malformed calls.
//   2. random sparse IoU matrices with few distinct values (ties), rows stored shuffled, random selections and thresholds that
//      equal some values, against a dense restatement of the reference's matching loop; malformed input — null pointers, negative
//      counts, row_start not starting at 0 or decreasing, columns outside [0, n), a NaN IoU, thresholds outside (0, 1] — is refused
//      with TD_ERR_INVALID and the outputs are left untouched.
// Exit status 0 and a final "ok" line on success; the first mismatch prints what differed and exits 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

[[noreturn]] void fail(const char* what, long long a = 0, long long b = 0) {
    std::printf("evaluation_check: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

// fmin / fmax drop a NaN; the rule's min and max hand it on (numpy's), and a NaN then fails the comparison
double nmin(double a, double b) { return (std::isnan(a) || std::isnan(b)) ? NAN : std::min(a, b); }
double nmax(double a, double b) { return (std::isnan(a) || std::isnan(b)) ? NAN : std::max(a, b); }

std::vector<double> random_boxes(std::mt19937& rng, int n, int flavour) {
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> b((size_t)n * 4);
    const double inf = std::numeric_limits<double>::infinity();
    for (int k = 0; k < n; ++k) {
        double x, y, w, h;
        if (flavour == 0) {                                           // a jittered field at map coordinates
            x = 412000.0 + 60.0 * u(rng), y = 5318000.0 + 60.0 * u(rng), w = 1.0 + 8.0 * u(rng), h = 1.0 + 8.0 * u(rng);
        } else {                                                      // a lattice: boxes touch, coincide, have zero width
            x = (double)(rng() % 8), y = (double)(rng() % 8), w = (double)(rng() % 4), h = (double)(rng() % 4);
        }
        double* p = &b[(size_t)k * 4];
        p[0] = x, p[1] = y, p[2] = x + w, p[3] = y + h;
        const unsigned r = rng() % 40;
        if (r < 4) p[r] = NAN;
        else if (r == 4) std::swap(p[0], p[2]);
        else if (r == 5) p[2] = inf;
        else if (r == 6) p[0] = -inf, p[1] = -inf, p[2] = inf, p[3] = inf;
        else if (r == 7) p[0] = inf, p[2] = inf;
    }
    return b;
}

void box_case(std::mt19937& rng, int n_a, int n_b, int flavour) {
    const std::vector<double> va = random_boxes(rng, n_a, flavour), vb = random_boxes(rng, n_b, flavour);
    auto a = exact(va), b = exact(vb);
    std::vector<std::vector<int32_t>> want(n_a);
    long long total = 0;
    for (int i = 0; i < n_a; ++i)
        for (int j = 0; j < n_b; ++j) {
            const double *p = &va[(size_t)i * 4], *q = &vb[(size_t)j * 4];
            if (nmin(p[2], q[2]) > nmax(p[0], q[0]) && nmin(p[3], q[3]) > nmax(p[1], q[1])) {
                want[i].push_back(j);
                ++total;
            }
        }
    std::unique_ptr<int32_t[]> counts(new int32_t[n_a]);
    if (td_box_pairs_ab(a.get(), n_a, b.get(), n_b, counts.get(), nullptr, 0) != TD_OK) fail("count call refused", n_a, n_b);
    for (int i = 0; i < n_a; ++i)
        if (counts[i] != (int32_t)want[i].size()) fail("row length differs", i, counts[i]);
    std::unique_ptr<int32_t[]> cols(new int32_t[total]);
    if (td_box_pairs_ab(a.get(), n_a, b.get(), n_b, counts.get(), cols.get(), total) != TD_OK) fail("fill call refused", n_a, n_b);
    long long at = 0;
    for (int i = 0; i < n_a; ++i)
        for (int32_t j : want[i])
            if (cols[at++] != j) fail("column differs (rows ascend)", i, j);
    if (total > 0 && td_box_pairs_ab(a.get(), n_a, b.get(), n_b, counts.get(), cols.get(), total - 1) != TD_ERR_CAPACITY)
        fail("a short cols buffer is not refused", total);
}

void box_malformed() {
    const std::vector<double> v = {0, 0, 1, 1};
    auto a = exact(v);
    std::unique_ptr<int32_t[]> counts(new int32_t[1]), cols(new int32_t[1]);
    if (td_box_pairs_ab(nullptr, 1, a.get(), 1, counts.get(), nullptr, 0) != TD_ERR_INVALID) fail("null boxes_a accepted");
    if (td_box_pairs_ab(a.get(), 1, nullptr, 1, counts.get(), nullptr, 0) != TD_ERR_INVALID) fail("null boxes_b accepted");
    if (td_box_pairs_ab(a.get(), 1, a.get(), 1, nullptr, nullptr, 0) != TD_ERR_INVALID) fail("null counts accepted");
    if (td_box_pairs_ab(a.get(), -1, a.get(), 1, counts.get(), nullptr, 0) != TD_ERR_INVALID) fail("n_a < 0 accepted");
    if (td_box_pairs_ab(a.get(), 1, a.get(), -1, counts.get(), nullptr, 0) != TD_ERR_INVALID) fail("n_b < 0 accepted");
    if (td_box_pairs_ab(a.get(), 1, a.get(), 1, counts.get(), cols.get(), -1) != TD_ERR_INVALID) fail("cols_cap < 0 accepted");
    if (td_box_pairs_ab(nullptr, 0, nullptr, 0, nullptr, nullptr, 0) != TD_OK) fail("two empty sets refused");
    if (td_box_pairs_ab(a.get(), 1, nullptr, 0, counts.get(), nullptr, 0) != TD_OK || counts[0] != 0) fail("an empty B refused");
}

void match_case(std::mt19937& rng, int m, int n, double density) {
    const double palette[] = {0.0, 0.125, 0.25, 0.3, 0.5, 0.625, 0.75, 1.0, 5e-324, 0.9999999999999999};
    const int shades = 2 + (int)(rng() % 9);
    std::bernoulli_distribution entry(density);
    std::vector<double> dense((size_t)m * n, -1.0);                  // -1: no entry
    std::vector<int64_t> row_start(m + 1, 0);
    std::vector<int32_t> cols;
    std::vector<double> iou;
    for (int i = 0; i < m; ++i) {
        std::vector<int32_t> row;
        for (int j = 0; j < n; ++j)
            if (entry(rng)) {
                dense[(size_t)i * n + j] = palette[rng() % shades];
                row.push_back(j);
            }
        if (rng() % 2) std::shuffle(row.begin(), row.end(), rng);    // the order inside a row does not matter
        for (int32_t j : row) {
            cols.push_back(j);
            iou.push_back(dense[(size_t)i * n + j]);
        }
        row_start[i + 1] = (int64_t)cols.size();
    }
    std::vector<uint8_t> selected(m);
    for (auto& s : selected) s = rng() % 5 != 0;
    const double thresholds[] = {0.125, 0.3, 0.5, 0.51, 1.0, 5e-324};
    const double t = thresholds[rng() % 6];
    // the reference's loop on the dense matrix: argmax over the unmatched candidates in ascending annotation order keeps the first
    std::vector<int32_t> want(m, -1);
    std::vector<double> want_iou(m, 0.0);
    std::vector<uint8_t> want_matched(n, 0);
    for (int i = 0; i < m; ++i) {
        if (!selected[i]) continue;
        int best = -1;
        for (int j = 0; j < n; ++j) {
            const double v = dense[(size_t)i * n + j];
            if (v < 0 || want_matched[j]) continue;
            if (best < 0 || v > dense[(size_t)i * n + best]) best = j;
        }
        if (best >= 0 && dense[(size_t)i * n + best] >= t) {
            want[i] = best;
            want_iou[i] = dense[(size_t)i * n + best];
            want_matched[best] = 1;
        }
    }
    auto rs = exact(row_start);
    auto cl = exact(cols);
    auto io = exact(iou);
    auto sel = exact(selected);
    std::unique_ptr<int32_t[]> of_pred(new int32_t[m]);
    std::unique_ptr<double[]> m_iou(new double[m]);
    std::unique_ptr<uint8_t[]> matched(new uint8_t[n]);
    std::fill(matched.get(), matched.get() + n, (uint8_t)7);
    if (td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), m, n, t, of_pred.get(), m_iou.get(), matched.get()) != TD_OK)
        fail("a well-formed matrix is refused", m, n);
    for (int i = 0; i < m; ++i)
        if (of_pred[i] != want[i] || m_iou[i] != want_iou[i]) fail("match differs", i, of_pred[i]);
    for (int j = 0; j < n; ++j)
        if (matched[j] != want_matched[j]) fail("ann_matched differs", j, matched[j]);
}

void match_malformed() {
    const std::vector<int64_t> row_start = {0, 2, 3};
    const std::vector<int32_t> cols = {0, 1, 1};
    const std::vector<double> iou = {0.5, 0.25, 0.75};
    const std::vector<uint8_t> selected = {1, 1};
    auto rs = exact(row_start);
    auto cl = exact(cols);
    auto io = exact(iou);
    auto sel = exact(selected);
    std::unique_ptr<int32_t[]> of_pred(new int32_t[2]);
    std::unique_ptr<double[]> m_iou(new double[2]);
    std::unique_ptr<uint8_t[]> matched(new uint8_t[2]);
    of_pred[0] = of_pred[1] = 77;
    auto refused = [&](const char* what, int st) {
        if (st != TD_ERR_INVALID) fail(what, st);
        if (of_pred[0] != 77 || of_pred[1] != 77) fail("a refused call wrote its outputs");
        if (!td_last_error() || !*td_last_error()) fail("a refused call left no message");
    };
    refused("null row_start", td_match_greedy(nullptr, cl.get(), io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("null cols", td_match_greedy(rs.get(), nullptr, io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("null iou", td_match_greedy(rs.get(), cl.get(), nullptr, sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("null selected", td_match_greedy(rs.get(), cl.get(), io.get(), nullptr, 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("null match_of_pred", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, 2, 0.3, nullptr, m_iou.get(), matched.get()));
    refused("null match_iou", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), nullptr, matched.get()));
    refused("null ann_matched", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), nullptr));
    refused("m < 0", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), -1, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("n < 0", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, -1, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    refused("a column outside [0, n)", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, 1, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    const double bad_t[] = {0.0, -0.5, 1.0000000000000002, NAN, std::numeric_limits<double>::infinity()};
    for (double t : bad_t)
        refused("a threshold outside (0, 1]", td_match_greedy(rs.get(), cl.get(), io.get(), sel.get(), 2, 2, t, of_pred.get(), m_iou.get(), matched.get()));
    for (const std::vector<int64_t>& bad : {std::vector<int64_t>{1, 2, 3}, std::vector<int64_t>{0, 3, 2}, std::vector<int64_t>{0, -1, 3}}) {
        auto brs = exact(bad);
        refused("a bad row_start", td_match_greedy(brs.get(), cl.get(), io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    }
    auto neg = exact(std::vector<int32_t>{0, -1, 1});
    refused("a negative column", td_match_greedy(rs.get(), neg.get(), io.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    auto nan_iou = exact(std::vector<double>{0.5, NAN, 0.75});
    refused("a NaN IoU", td_match_greedy(rs.get(), cl.get(), nan_iou.get(), sel.get(), 2, 2, 0.3, of_pred.get(), m_iou.get(), matched.get()));
    // the empty shapes are served
    const std::vector<int64_t> zero = {0};
    auto zrs = exact(zero);
    if (td_match_greedy(zrs.get(), nullptr, nullptr, nullptr, 0, 2, 0.3, nullptr, nullptr, matched.get()) != TD_OK || matched[0] || matched[1])
        fail("no predictions refused");
    const std::vector<int64_t> empty_rows = {0, 0, 0};
    auto ers = exact(empty_rows);
    if (td_match_greedy(ers.get(), nullptr, nullptr, sel.get(), 2, 0, 0.3, of_pred.get(), m_iou.get(), nullptr) != TD_OK || of_pred[0] != -1)
        fail("no annotations refused");
}

}  // namespace

int main() {
    std::mt19937 rng(20251021);
    const int sizes[][2] = {{0, 0}, {0, 5}, {5, 0}, {1, 1}, {1, 40}, {40, 1}, {37, 53}, {120, 90}, {300, 257}};
    int cases = 0;
    for (const auto& s : sizes)
        for (int flavour = 0; flavour < 2; ++flavour)
            for (int rep = 0; rep < 4; ++rep, ++cases) box_case(rng, s[0], s[1], flavour);
    box_malformed();
    int matches = 0;
    for (int trial = 0; trial < 400; ++trial, ++matches)
        match_case(rng, 1 + (int)(rng() % 60), 1 + (int)(rng() % 40), trial % 2 ? 0.3 : 0.06);
    match_malformed();
    std::printf("evaluation_check: ok (%d box cases, %d matrices)\n", cases, matches);
    return 0;
}
