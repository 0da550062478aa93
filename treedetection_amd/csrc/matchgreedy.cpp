// The matching loop of the evaluation (reference supplementary/evaluation_compute_scores.py calculate_iou) over the sparse IoU
// matrix of one image instead of a shapely overlay per prediction and threshold: predictions in index order, each selected one
// takes the still unmatched annotation of its row with the largest IoU (the lowest annotation index among equals: np.argmax keeps
// the first) when that IoU is >= t. Sequential by nature (an earlier prediction takes an annotation away from a later, better
// one); O(rows + entries). Host code.
#include "common.h"

#include <cmath>
#include <cstring>

extern "C" int td_match_greedy(const int64_t* row_start, const int32_t* cols, const double* iou, const uint8_t* selected, int m, int n,
                               double t, int32_t* match_of_pred, double* match_iou, uint8_t* ann_matched) {
    if (m < 0 || n < 0) {
        td_set_error("td_match_greedy: m = %d, n = %d, a count is negative", m, n);
        return TD_ERR_INVALID;
    }
    if (!row_start || (m > 0 && (!selected || !match_of_pred || !match_iou)) || (n > 0 && !ann_matched)) {
        td_set_error("td_match_greedy: null pointer");
        return TD_ERR_INVALID;
    }
    if (!(t > 0.0 && t <= 1.0)) {
        td_set_error("td_match_greedy: the IoU threshold %g is not in (0, 1]", t);
        return TD_ERR_INVALID;
    }
    int64_t prev = row_start[0];
    if (prev != 0) {
        td_set_error("td_match_greedy: row_start[0] = %lld, must be 0", (long long)prev);
        return TD_ERR_INVALID;
    }
    for (int i = 0; i < m; ++i) {
        if (row_start[i + 1] < prev) {
            td_set_error("td_match_greedy: row_start decreases at row %d", i);
            return TD_ERR_INVALID;
        }
        prev = row_start[i + 1];
    }
    if (prev > 0 && (!cols || !iou)) {
        td_set_error("td_match_greedy: null pointer (cols or iou of %lld entries)", (long long)prev);
        return TD_ERR_INVALID;
    }
    for (int64_t e = 0; e < prev; ++e) {
        if (cols[e] < 0 || cols[e] >= n) {
            td_set_error("td_match_greedy: cols[%lld] = %d outside [0, %d)", (long long)e, cols[e], n);
            return TD_ERR_INVALID;
        }
        if (std::isnan(iou[e])) {
            td_set_error("td_match_greedy: iou[%lld] is NaN", (long long)e);
            return TD_ERR_INVALID;
        }
    }
    if (n > 0) std::memset(ann_matched, 0, (size_t)n);
    for (int i = 0; i < m; ++i) {
        match_of_pred[i] = -1;
        match_iou[i] = 0.0;
        if (!selected[i]) continue;
        int best = -1;
        double best_iou = 0.0;
        for (int64_t e = row_start[i]; e < row_start[i + 1]; ++e) {
            const int j = cols[e];
            if (ann_matched[j]) continue;
            if (best < 0 || iou[e] > best_iou || (iou[e] == best_iou && j < best)) {
                best = j;
                best_iou = iou[e];
            }
        }
        if (best >= 0 && best_iou >= t) {
            match_of_pred[i] = best;
            match_iou[i] = best_iou;
            ann_matched[best] = 1;
        }
    }
    return TD_OK;
}
