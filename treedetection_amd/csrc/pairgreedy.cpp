// The greedy pass of the crown stage's de-duplication (reference TreeDetection/postprocessing.py:386-406) over sparse rows: the
// connected pairs come from td_crown_pairs_count / td_crown_pairs_fill as CSR lists instead of an N x N mask. Sequential by
// nature (a removed crown is skipped as a group's owner but still votes in later groups); O(n + edges). Host code.
#include "common.h"

#include <cstring>

namespace {

// IEEE half bit pattern → float (exact); confidences are compared as numpy compares float16 values
float half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
    if (exp == 0x1fu) {
        bits = sign | 0x7f800000u | (man << 13);
    } else if (exp != 0) {
        bits = sign | ((exp + 112u) << 23) | (man << 13);
    } else if (man == 0) {
        bits = sign;
    } else {                                             // subnormal: man * 2^-24
        int shift = 0;
        while (!(man & 0x400u)) {
            man <<= 1;
            ++shift;
        }
        bits = sign | ((uint32_t)(113 - shift) << 23) | ((man & 0x3ffu) << 13);
    }
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
}

}  // namespace

extern "C" int td_crown_pairs_greedy(const int64_t* row_start, const int32_t* cols, const uint16_t* conf_f16,
                                     const uint8_t* self_connected, int n, uint8_t* removed) {
    if (!row_start || !conf_f16 || !removed || n < 0 || (n > 0 && row_start[n] > 0 && !cols)) {
        td_set_error("td_crown_pairs_greedy: null pointer or n < 0");
        return TD_ERR_INVALID;
    }
    int64_t prev = n > 0 ? row_start[0] : 0;
    if (prev != 0) {
        td_set_error("td_crown_pairs_greedy: row_start[0] = %lld, must be 0", (long long)prev);
        return TD_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        if (row_start[i + 1] < prev) {
            td_set_error("td_crown_pairs_greedy: row_start decreases at row %d", i);
            return TD_ERR_INVALID;
        }
        prev = row_start[i + 1];
    }
    for (int64_t e = 0; e < prev; ++e)
        if (cols[e] < 0 || cols[e] >= n) {
            td_set_error("td_crown_pairs_greedy: cols[%lld] = %d outside [0, %d)", (long long)e, cols[e], n);
            return TD_ERR_INVALID;
        }
    std::memset(removed, 0, (size_t)n);
    for (int i = 0; i < n; ++i) {
        if (removed[i]) continue;
        // the reference takes argmax over the ascending list of the mask's row with i appended: the first of the highest
        // confidences in that order. Within the row that is the smallest index (whatever order the row is stored in); the
        // appended i wins only when it is strictly higher — unless the mask's diagonal is set, which puts i into the row too.
        int best = -1;
        float best_conf = 0.f;
        auto offer = [&](int j) {
            const float c = half_bits_to_float(conf_f16[j]);
            if (best < 0 || c > best_conf || (c == best_conf && j < best)) {
                best = j;
                best_conf = c;
            }
        };
        for (int64_t e = row_start[i]; e < row_start[i + 1]; ++e) offer(cols[e]);
        if (!self_connected || self_connected[i]) offer(i);
        if (best < 0 || half_bits_to_float(conf_f16[i]) > best_conf) best = i;
        for (int64_t e = row_start[i]; e < row_start[i + 1]; ++e)
            if (cols[e] != best) removed[cols[e]] = 1;
        if (best != i) removed[i] = 1;
    }
    return TD_OK;
}
