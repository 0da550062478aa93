// Zonal statistics of a raster over a crown's OUTLINE (td_crown_zonal_dev, crownzonal.hip; td_crown_zonal, crownzonal_host.cpp): the
// rule that says which pixels belong to a crown, the box that is searched for them and the order in which values displace each
// other — written once for host and device (TD_GEOM_HD), plain IEEE float64, built with -ffp-contract=off on both sides.
//
// Membership. Pixel (row, col) of the whole raster — no window, no row / column swap: those belong to the circle path (crown.hip) —
// has the centre P = pixel_centre(); it belongs to the crown iff tdgeom::point_in_query(ring, n, P) != 0 on the crown's exterior
// ring as stored (float64, closed): even-odd over all edges, half-open in y, the boundary inside, every sign from
// tdgeom::orientation() with its double-double fallback. Either winding; a ring that crosses itself is even-odd like any other.
//
// The box. A centre that passes lies inside the ring's float64 bounding box [x0, x1] x [y0, y1] — exactly: the comparisons are on
// the doubles the orientation sees, a point beyond the box has no edge envelope around it and an even number of crossings. So the
// pixels outside pixel_box() — the indices whose centres can reach that box, with a margin for the rounding of the inverse map —
// need no test, and neither does a centre that fails the comparison with the box itself. Both only save work: no answer depends on them.
#pragma once
#include "geom_predicates.h"

namespace tdzonal {

using tdgeom::Pt;

struct Affine {
    double a, b, c, d, e, f;
};

// centre of pixel (row, col): x = (a * (col + 0.5) + b * (row + 0.5)) + c, y = (d * (col + 0.5) + e * (row + 0.5)) + f
TD_GEOM_HD inline Pt pixel_centre(const Affine& t, int row, int col) {
    const double u = (double)col + 0.5, v = (double)row + 0.5;
    return {(t.a * u + t.b * v) + t.c, (t.d * u + t.e * v) + t.f};
}

// b == 0 and d == 0: y is the same along a row (d * u is a zero, which changes nothing it is added to) and x along a column
TD_GEOM_HD inline bool axis_aligned(const Affine& t) { return t.b == 0.0 && t.d == 0.0; }

TD_GEOM_HD inline bool is_finite(double v) { return v - v == 0.0; }

// The indices i of [0, n) whose centre coordinate (s * (i + 0.5)) + o can lie in [lo, hi] → [*i0, *i1], empty when *i0 > *i1.
// s != 0. A superset: the inverse (t - o) / s - 0.5 is off by a few units in the last place of (|t| + |o|) / |s| — in index units —
// and so is the centre as pixel_centre rounds it; the margin is one index plus 32 times that. A NaN anywhere gives the whole range.
TD_GEOM_HD inline void index_range(double lo, double hi, double s, double o, int n, int* i0, int* i1) {
    double u0 = (lo - o) / s - 0.5, u1 = (hi - o) / s - 0.5;
    if (u0 > u1) {
        const double t = u0;
        u0 = u1;
        u1 = t;
    }
    const double m = 1.0 + (std::fabs(lo) + std::fabs(hi) + std::fabs(o)) / std::fabs(s) * 0x1p-48;
    const double f0 = std::floor(u0 - m), f1 = std::ceil(u1 + m);
    *i0 = f0 > 0.0 ? (f0 >= (double)n ? n : (int)f0) : 0;
    *i1 = f1 < (double)(n - 1) ? (f1 < 0.0 ? -1 : (int)f1) : n - 1;
}

struct Box {
    int r0, r1, c0, c1;          // rows r0 .. r1 and columns c0 .. c1, inside the raster; empty when r0 > r1 or c0 > c1
};

// The pixels whose centres can lie in [x0, x1] x [y0, y1]. Axis-aligned: one index_range per axis. Rotated: the box of the four
// corners taken back through the inverse transform (a point of the box maps inside their parallelogram), the margin grown by the
// rounding of the two products that meet in each coordinate. A transform without an inverse gives the whole raster.
TD_GEOM_HD inline Box pixel_box(const Affine& t, double x0, double y0, double x1, double y1, int rows, int cols) {
    Box B{0, rows - 1, 0, cols - 1};
    if (axis_aligned(t)) {
        if (t.a != 0.0) index_range(x0, x1, t.a, t.c, cols, &B.c0, &B.c1);
        if (t.e != 0.0) index_range(y0, y1, t.e, t.f, rows, &B.r0, &B.r1);
        return B;
    }
    const double det = t.a * t.e - t.b * t.d;
    if (det == 0.0 || !is_finite(det)) return B;
    const double inf = __builtin_inf();
    double ulo = inf, uhi = -inf, vlo = inf, vhi = -inf;
    for (int k = 0; k < 4; ++k) {
        const double dx = ((k & 1) ? x1 : x0) - t.c, dy = ((k & 2) ? y1 : y0) - t.f;
        const double u = (t.e * dx - t.b * dy) / det - 0.5, v = (t.a * dy - t.d * dx) / det - 0.5;
        ulo = u < ulo ? u : ulo;
        uhi = u > uhi ? u : uhi;
        vlo = v < vlo ? v : vlo;
        vhi = v > vhi ? v : vhi;
    }
    const double mag = std::fabs(x0) + std::fabs(x1) + std::fabs(y0) + std::fabs(y1) + std::fabs(t.c) + std::fabs(t.f);
    const double mu = 1.0 + (std::fabs(t.e) + std::fabs(t.b)) * mag / std::fabs(det) * 0x1p-48;
    const double mv = 1.0 + (std::fabs(t.a) + std::fabs(t.d)) * mag / std::fabs(det) * 0x1p-48;
    const double c0 = std::floor(ulo - mu), c1 = std::ceil(uhi + mu), r0 = std::floor(vlo - mv), r1 = std::ceil(vhi + mv);
    B.c0 = c0 > 0.0 ? (c0 >= (double)cols ? cols : (int)c0) : 0;
    B.c1 = c1 < (double)(cols - 1) ? (c1 < 0.0 ? -1 : (int)c1) : cols - 1;
    B.r0 = r0 > 0.0 ? (r0 >= (double)rows ? rows : (int)r0) : 0;
    B.r1 = r1 < (double)(rows - 1) ? (r1 < 0.0 ? -1 : (int)r1) : rows - 1;
    return B;
}

TD_GEOM_HD inline bool in_bounds(const Pt& p, double x0, double y0, double x1, double y1) {
    return p.x >= x0 && p.x <= x1 && p.y >= y0 && p.y <= y1;
}

// The order of the maximum — crown.hip's max_takes, numpy's argmax: does (v, lin) displace the running (vmax, imax)? A NaN beats
// every number; among NaNs, and among equal numbers (+0.0 and -0.0 are equal), the lower row-major position wins.
TD_GEOM_HD inline bool max_takes(float v, long long lin, float vmax, long long imax) {
    if (imax < 0) return true;
    const bool v_nan = v != v, m_nan = vmax != vmax;
    if (v_nan || m_nan) return v_nan && (!m_nan || lin < imax);
    return v > vmax || (v == vmax && lin < imax);
}

// The order of the minimum: crown.hip's min_nan — a NaN, once met, stays; a smaller number displaces — applied in row-major order,
// which is what carrying the position says: among equal numbers (a zero of either sign) the first one stays.
TD_GEOM_HD inline bool min_takes(float v, long long lin, float vmin, long long imin) {
    if (imin < 0) return true;
    const bool v_nan = v != v, m_nan = vmin != vmin;
    if (v_nan || m_nan) return v_nan && (!m_nan || lin < imin);
    return v < vmin || (v == vmin && lin < imin);
}

}  // namespace tdzonal
