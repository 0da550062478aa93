// The host twin of td_treetops_dev (treetops.hip): the two smoothing passes, the window maximum and the comparison from the same
// header (treetops.h), over whole rasters on one thread, for any radius and window. It serves the parameters over the kernel's caps,
// the host path of treetops.find_treetops (device=None) and the CPU tests; marks and smoothed equal the device's bit for bit. Host code.
#include "common.h"
#include "treetops.h"

#include <new>
#include <vector>

using namespace tdtops;

extern "C" td_status td_treetops(const float* raster, int rows, int cols, const double* weights, int radius, int window, float floor,
                                 uint8_t* marks, float* smoothed, int32_t* counts) {
    TD_REQUIRE(raster && weights && marks, "td_treetops: null pointer");
    if (const char* why = refusal(rows, cols, weights, radius, window, floor)) {
        td_set_error("td_treetops: %s (a %d x %d raster, radius %d, window %d)", why, rows, cols, radius, window);
        return TD_ERR_INVALID;
    }
    const int r = radius, h = window / 2;
    const size_t n = (size_t)rows * cols;
    std::vector<float> a, b;
    try {
        a.resize(n);
        b.resize(n);
    } catch (const std::bad_alloc&) {
        td_set_error("td_treetops: no memory for two %d x %d float32 rasters", rows, cols);
        return TD_ERR_INVALID;
    }
    // axis 0: a[row][col] over raster[row + ii][col]
    std::vector<int> idx((size_t)2 * r + 1);
    for (int row = 0; row < rows; ++row) {
        for (int ii = -r; ii <= r; ++ii) idx[ii + r] = reflect((long long)row + ii, rows);
        for (int col = 0; col < cols; ++col)
            a[(size_t)row * cols + col] = smooth_one(weights, r, [&](int ii) { return raster[(size_t)idx[ii + r] * cols + col]; });
    }
    // axis 1: b[row][col] over a[row][col + ii]
    for (int row = 0; row < rows; ++row) {
        const float* line = a.data() + (size_t)row * cols;
        for (int col = 0; col < cols; ++col)
            b[(size_t)row * cols + col] = smooth_one(weights, r, [&](int ii) { return line[reflect((long long)col + ii, cols)]; });
    }
    // the window maximum, separable, over the in-range pixels: a = the maximum down the columns, then along the rows
    for (int row = 0; row < rows; ++row) {
        const int r0 = row - h < 0 ? 0 : row - h, r1 = (long long)row + h > rows - 1 ? rows - 1 : row + h;
        for (int col = 0; col < cols; ++col) {
            float m = b[(size_t)r0 * cols + col];
            for (int q = r0 + 1; q <= r1; ++q) m = fmax_nan(m, b[(size_t)q * cols + col]);
            a[(size_t)row * cols + col] = m;
        }
    }
    for (int row = 0; row < rows; ++row) {
        const float* line = a.data() + (size_t)row * cols;
        int32_t in_row = 0;
        for (int col = 0; col < cols; ++col) {
            const int c0 = col - h < 0 ? 0 : col - h, c1 = (long long)col + h > cols - 1 ? cols - 1 : col + h;
            float m = line[c0];
            for (int q = c0 + 1; q <= c1; ++q) m = fmax_nan(m, line[q]);
            const float s = b[(size_t)row * cols + col];
            const bool top = is_top(s, m, floor);
            marks[(size_t)row * cols + col] = top ? 1 : 0;
            in_row += top;
            if (smoothed) smoothed[(size_t)row * cols + col] = s;
        }
        if (counts) counts[row] = in_row;
    }
    return TD_OK;
}
