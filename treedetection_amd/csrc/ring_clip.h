// The exact-formula intersection area of two simple polygon rings, one source for the wave (ringiou.hip) and for the host
// (ringiou_host.cpp). Float64 throughout, every operation rounded on its own (-ffp-contract=off in both builds), IEEE division.
//
// Fan decomposition about a common origin O: with s_i = cross(p_i - O, p_i+1 - O), t_j likewise for Q, and sigma the sign of a
// ring's own signed area,
//     area(P n Q) = sigma_P sigma_Q * sum_i sum_j sgn(s_i) sgn(t_j) * area(tri(O, p_i, p_i+1) n tri(O, q_j, q_j+1)),
// for any simple ring, convex or not, in either winding (the signed fan triangles of a ring add up to its indicator function
// times sigma, and the product of two such sums is the indicator of the intersection). A fan triangle with s = 0 is skipped.
// Each term: one triangle, turned counter-clockwise, clipped by the three half-planes of the other (Sutherland-Hodgman: at most
// 3 + 3 vertices), then the shoelace sum. The polygon under the clip is held in fixed slots that are written through selects —
// no indexed array, so on the device it stays in registers — and every loop has a fixed trip count.
//
// Prescribed so that host, device and tests agree:
//   O        = the centre of the intersection of the two rings' float64 bounding boxes, ((max(minx) + min(maxx)) / 2, same in y);
//              vertices are used as v - O; a box intersection of non-positive width or height gives +0 and no clip runs.
//   order    term t = i * n + j goes to lane t mod 64; a lane adds its terms in ascending t; the 64 partial sums meet in a
//              butterfly over xor 32, 16, 8, 4, 2, 1 (rc_butterfly: what 64 lanes do with __shfl_xor, emulated on the host).
//   areas    the shoelace sum of a ring on v - O in the same order: edge k to lane k mod 64, the same butterfly, times 1/2.
//   result   inter clamped to [0, min(|area_P|, |area_Q|)], |area_P|, |area_Q|.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define TD_RC_HD __host__ __device__ inline
#define TD_RC_UNROLL _Pragma("unroll")
#else
#define TD_RC_HD static inline
#define TD_RC_UNROLL
#endif

constexpr int RC_LANES = 64;

TD_RC_HD bool rc_finite(double v) { return v - v == 0.0; }         // false for NaN and both infinities

TD_RC_HD double rc_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// Up to six vertices in fixed slots. put() appends through selects; a seventh vertex — which only rounding noise on a polygon
// that has collapsed onto the clip line could ask for — is dropped.
struct RcPoly {
    double x[6], y[6];
    int n;
};

TD_RC_HD void rc_put(RcPoly& o, double px, double py) {
    TD_RC_UNROLL
    for (int k = 0; k < 6; ++k) {
        const bool here = o.n == k;
        o.x[k] = here ? px : o.x[k];
        o.y[k] = here ? py : o.y[k];
    }
    o.n = o.n < 6 ? o.n + 1 : 6;
}

// `in` (at most MAXIN vertices, counter-clockwise) cut by the half-plane to the left of e0 -> e1 (the line included)
template <int MAXIN>
TD_RC_HD void rc_clip_halfplane(const RcPoly& in, double e0x, double e0y, double e1x, double e1y, RcPoly& out) {
    const double ex = e1x - e0x, ey = e1y - e0y;
    double d[MAXIN];
    TD_RC_UNROLL
    for (int k = 0; k < MAXIN; ++k) d[k] = rc_cross(ex, ey, in.x[k] - e0x, in.y[k] - e0y);
    out.n = 0;
    TD_RC_UNROLL
    for (int k = 0; k < 6; ++k) out.x[k] = out.y[k] = 0.0;
    TD_RC_UNROLL
    for (int k = 0; k < MAXIN; ++k) {
        if (k < in.n) {
            const bool wrap = k + 1 >= in.n;
            const double px = in.x[k], py = in.y[k], dp = d[k];
            const double qx = wrap ? in.x[0] : in.x[k + 1 < MAXIN ? k + 1 : 0];
            const double qy = wrap ? in.y[0] : in.y[k + 1 < MAXIN ? k + 1 : 0];
            const double dq = wrap ? d[0] : d[k + 1 < MAXIN ? k + 1 : 0];
            const bool pin = dp >= 0.0, qin = dq >= 0.0;
            if (pin) rc_put(out, px, py);
            if (pin != qin) {
                const double u = dp / (dp - dq);
                rc_put(out, px + (qx - px) * u, py + (qy - py) * u);
            }
        }
    }
}

// area(tri(O, a, b) n tri(O, c, d)) with O the origin, unsigned up to rounding; s = cross(a, b) and t = cross(c, d), both non-zero
TD_RC_HD double rc_tri_tri_area(double ax, double ay, double bx, double by, double s, double cx, double cy, double dx, double dy,
                                double t) {
    RcPoly p0, p1, p2, p3;
    const bool fa = s < 0.0, fc = t < 0.0;           // turn both counter-clockwise
    p0.n = 3;
    p0.x[0] = 0.0, p0.y[0] = 0.0;
    p0.x[1] = fa ? bx : ax, p0.y[1] = fa ? by : ay;
    p0.x[2] = fa ? ax : bx, p0.y[2] = fa ? ay : by;
    TD_RC_UNROLL
    for (int k = 3; k < 6; ++k) p0.x[k] = p0.y[k] = 0.0;
    const double c1x = fc ? dx : cx, c1y = fc ? dy : cy, c2x = fc ? cx : dx, c2y = fc ? cy : dy;
    rc_clip_halfplane<3>(p0, 0.0, 0.0, c1x, c1y, p1);
    rc_clip_halfplane<4>(p1, c1x, c1y, c2x, c2y, p2);
    rc_clip_halfplane<5>(p2, c2x, c2y, 0.0, 0.0, p3);
    double sum = 0.0;
    TD_RC_UNROLL
    for (int k = 0; k < 6; ++k) {
        if (k < p3.n) {
            const bool wrap = k + 1 >= p3.n;
            const double qx = wrap ? p3.x[0] : p3.x[k + 1 < 6 ? k + 1 : 0];
            const double qy = wrap ? p3.y[0] : p3.y[k + 1 < 6 ? k + 1 : 0];
            sum += rc_cross(p3.x[k], p3.y[k], qx, qy);
        }
    }
    return 0.5 * sum;
}

// term (i, j) of the double sum, sign included; p / q: the rings as v - O, m / n their vertex counts
TD_RC_HD double rc_term(const double* px, const double* py, int m, const double* qx, const double* qy, int n, int i, int j) {
    const int i1 = i + 1 == m ? 0 : i + 1, j1 = j + 1 == n ? 0 : j + 1;
    const double ax = px[i], ay = py[i], bx = px[i1], by = py[i1];
    const double cx = qx[j], cy = qy[j], dx = qx[j1], dy = qy[j1];
    const double s = rc_cross(ax, ay, bx, by), t = rc_cross(cx, cy, dx, dy);
    if (s == 0.0 || t == 0.0) return 0.0;
    const double a = rc_tri_tri_area(ax, ay, bx, by, s, cx, cy, dx, dy, t);
    return (s < 0.0) != (t < 0.0) ? -a : a;
}

// shoelace term k of a ring given as v - O
TD_RC_HD double rc_edge_cross(const double* x, const double* y, int m, int k) {
    const int k1 = k + 1 == m ? 0 : k + 1;
    return rc_cross(x[k], y[k], x[k1], y[k1]);
}

// the 64 partial sums combined as the wave combines them: every lane ends with the same total
TD_RC_HD double rc_butterfly(double* part) {
    for (int d = RC_LANES / 2; d >= 1; d >>= 1) {
        double next[RC_LANES];
        for (int l = 0; l < RC_LANES; ++l) next[l] = part[l] + part[l ^ d];
        for (int l = 0; l < RC_LANES; ++l) part[l] = next[l];
    }
    return part[0];
}

// the three results from the three sums (double sum of terms, shoelace sums of P and Q)
TD_RC_HD void rc_finish(double terms, double shoe_p, double shoe_q, double* out) {
    const double ap = 0.5 * shoe_p, aq = 0.5 * shoe_q;
    const double abs_p = (ap < 0.0 ? -ap : ap) + 0.0, abs_q = (aq < 0.0 ? -aq : aq) + 0.0;      // (+ 0.0: -0 becomes +0)
    const double cap = abs_p < abs_q ? abs_p : abs_q;
    double inter = (ap < 0.0) != (aq < 0.0) ? -terms : terms;
    inter = inter > 0.0 ? inter : 0.0;                // (also turns -0 into +0)
    inter = inter < cap ? inter : cap;
    out[0] = inter;
    out[1] = abs_p;
    out[2] = abs_q;
}

// ---- the whole pair on the host: what one wave does, on emulated lanes ---------------------------------------------------------
// xa / xb: the open rings as (x, y) pairs, m, n >= 3, every coordinate finite; px .. qy: scratch of m / n doubles each
TD_RC_HD void rc_pair_host(const double* xa, int m, const double* xb, int n, double* px, double* py, double* qx, double* qy,
                           double* out) {
    double lo[2][2], hi[2][2];
    for (int r = 0; r < 2; ++r) {
        const double* v = r ? xb : xa;
        const int cnt = r ? n : m;
        lo[r][0] = hi[r][0] = v[0];
        lo[r][1] = hi[r][1] = v[1];
        for (int k = 1; k < cnt; ++k)
            for (int c = 0; c < 2; ++c) {
                const double w = v[2 * k + c];
                lo[r][c] = w < lo[r][c] ? w : lo[r][c];
                hi[r][c] = w > hi[r][c] ? w : hi[r][c];
            }
    }
    const double x0 = lo[0][0] > lo[1][0] ? lo[0][0] : lo[1][0], x1 = hi[0][0] < hi[1][0] ? hi[0][0] : hi[1][0];
    const double y0 = lo[0][1] > lo[1][1] ? lo[0][1] : lo[1][1], y1 = hi[0][1] < hi[1][1] ? hi[0][1] : hi[1][1];
    const double ox = (x0 + x1) / 2.0, oy = (y0 + y1) / 2.0;
    for (int k = 0; k < m; ++k) px[k] = xa[2 * k] - ox, py[k] = xa[2 * k + 1] - oy;
    for (int k = 0; k < n; ++k) qx[k] = xb[2 * k] - ox, qy[k] = xb[2 * k + 1] - oy;
    double part[RC_LANES];
    for (int l = 0; l < RC_LANES; ++l) part[l] = 0.0;
    for (int k = 0; k < m; ++k) part[k % RC_LANES] += rc_edge_cross(px, py, m, k);
    const double shoe_p = rc_butterfly(part);
    for (int l = 0; l < RC_LANES; ++l) part[l] = 0.0;
    for (int k = 0; k < n; ++k) part[k % RC_LANES] += rc_edge_cross(qx, qy, n, k);
    const double shoe_q = rc_butterfly(part);
    double terms = 0.0;
    if (x1 > x0 && y1 > y0) {
        for (int l = 0; l < RC_LANES; ++l) part[l] = 0.0;
        int i = 0, j = 0;
        for (int64_t t = 0; t < (int64_t)m * n; ++t) {
            part[t % RC_LANES] += rc_term(px, py, m, qx, qy, n, i, j);
            if (++j == n) j = 0, ++i;
        }
        terms = rc_butterfly(part);
    }
    rc_finish(terms, shoe_p, shoe_q, out);
}
