// Exact-sign planar predicates shared by the geometry code (geometry.cpp, region.cpp): orientation of three points
// with a floating-point filter backed by double-double arithmetic — the scheme GEOS uses
// (CGAlgorithmsDD::orientationIndex), so collinear / touching configurations are classified the same way.
// Below it, what the outline predicates are made of (region.cpp on the host, regionrelate.hip on the device): the rule of one
// region edge against a point, segments_meet, meet_params, point_in_query. Every function compiles for host and device
// (TD_GEOM_HD) and is plain IEEE float64 with one explicit fma; both sides are built with -ffp-contract=off, so a meeting
// parameter or a midpoint has the same bits wherever it is formed.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TD_GEOM_HD __host__ __device__
#else
#define TD_GEOM_HD
#endif

namespace tdgeom {

struct DD {
    double hi, lo;
};
TD_GEOM_HD inline DD two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
TD_GEOM_HD inline DD two_prod(double a, double b) {
    const double p = a * b;
    return {p, std::fma(a, b, -p)};
}
TD_GEOM_HD inline DD dd_add(DD a, DD b) {
    DD s = two_sum(a.hi, b.hi);
    DD t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = two_sum(s.hi, s.lo);     // renormalise
    s.lo += t.lo;
    return two_sum(s.hi, s.lo);
}
TD_GEOM_HD inline DD dd_neg(DD a) { return {-a.hi, -a.lo}; }
TD_GEOM_HD inline DD dd_mul(DD a, DD b) {
    DD p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return two_sum(p.hi, p.lo);
}
TD_GEOM_HD inline DD dd_diff(double a, double b) { return two_sum(a, -b); }   // exact a - b

// sign of the orientation of q relative to the directed line p1 -> p2 (+1 left, -1 right, 0 collinear)
TD_GEOM_HD inline int orientation(double p1x, double p1y, double p2x, double p2y, double qx, double qy) {
    // fast filter: the double determinant decides unless it is within its rounding error bound
    const double detleft = (p1x - qx) * (p2y - qy);
    const double detright = (p1y - qy) * (p2x - qx);
    const double det = detleft - detright;
    const auto sign = [](double v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); };
    double detsum;
    if (detleft > 0.0) {
        if (detright <= 0.0) return sign(det);
        detsum = detleft + detright;
    } else if (detleft < 0.0) {
        if (detright >= 0.0) return sign(det);
        detsum = -detleft - detright;
    } else {
        return sign(det);
    }
    const double errbound = 1e-15 * detsum;
    if (det >= errbound || -det >= errbound) return sign(det);
    // double-double evaluation of (p2 - p1) x (q - p2)
    const DD dx1 = dd_diff(p2x, p1x), dy1 = dd_diff(p2y, p1y);
    const DD dx2 = dd_diff(qx, p2x), dy2 = dd_diff(qy, p2y);
    const DD d = dd_add(dd_mul(dx1, dy2), dd_neg(dd_mul(dy1, dx2)));
    if (d.hi > 0 || (d.hi == 0 && d.lo > 0)) return 1;
    if (d.hi < 0 || (d.hi == 0 && d.lo < 0)) return -1;
    return 0;
}

struct Pt {
    double x, y;
    TD_GEOM_HD bool operator==(const Pt& o) const { return x == o.x && y == o.y; }
};

TD_GEOM_HD inline bool env_has(const Pt& a, const Pt& b, const Pt& q) {   // q inside the envelope of segment (a, b)
    return q.x >= std::fmin(a.x, b.x) && q.x <= std::fmax(a.x, b.x) && q.y >= std::fmin(a.y, b.y) && q.y <= std::fmax(a.y, b.y);
}
TD_GEOM_HD inline bool env_overlap(const Pt& p1, const Pt& p2, const Pt& q1, const Pt& q2) {
    return !(std::fmin(q1.x, q2.x) > std::fmax(p1.x, p2.x) || std::fmax(q1.x, q2.x) < std::fmin(p1.x, p2.x) ||
             std::fmin(q1.y, q2.y) > std::fmax(p1.y, p2.y) || std::fmax(q1.y, q2.y) < std::fmin(p1.y, p2.y));
}

// One region edge (a, b) against point p, for the crossing count of a horizontal ray from p to +x with the half-open rule on y:
// 0 the edge says nothing, 1 p lies on it, 2 the ray crosses it.
TD_GEOM_HD inline int edge_point_rule(const Pt& a, const Pt& b, const Pt& p) {
    const double lo = std::fmin(a.y, b.y), hi = std::fmax(a.y, b.y);
    if (p.y < lo || p.y > hi) return 0;
    if (std::fmax(a.x, b.x) < p.x) return 0;
    const int o = orientation(a.x, a.y, b.x, b.y, p.x, p.y);
    if (o == 0 && env_has(a, b, p)) return 1;
    if ((a.y <= p.y) != (b.y <= p.y)) {                  // half-open: counts an edge once at a shared vertex
        const bool up = a.y <= p.y;                      // a below-or-level, b above
        if ((up && o > 0) || (!up && o < 0)) return 2;
    }
    return 0;
}

// does segment (p1,p2) meet segment (q1,q2) at all (touching counts)?
TD_GEOM_HD inline bool segments_meet(const Pt& p1, const Pt& p2, const Pt& q1, const Pt& q2) {
    if (!env_overlap(p1, p2, q1, q2)) return false;
    const int a = orientation(p1.x, p1.y, p2.x, p2.y, q1.x, q1.y);
    const int b = orientation(p1.x, p1.y, p2.x, p2.y, q2.x, q2.y);
    if ((a > 0 && b > 0) || (a < 0 && b < 0)) return false;
    const int c = orientation(q1.x, q1.y, q2.x, q2.y, p1.x, p1.y);
    const int d = orientation(q1.x, q1.y, q2.x, q2.y, p2.x, p2.y);
    if ((c > 0 && d > 0) || (c < 0 && d < 0)) return false;
    return true;     // collinear pairs reach here only with overlapping envelopes, i.e. they share a point
}

// projection parameter of q on (p1, p1 + d), clamped to [0, 1]; len2 = |d|^2
TD_GEOM_HD inline double meet_param_of(const Pt& p1, double dx, double dy, double len2, const Pt& q) {
    const double v = len2 > 0 ? ((q.x - p1.x) * dx + (q.y - p1.y) * dy) / len2 : 0.0;
    return v < 0 ? 0.0 : (v > 1 ? 1.0 : v);
}

// parameters t in [0,1] along (p1,p2) where it meets (q1,q2): none, one point, or the two ends of a collinear overlap
TD_GEOM_HD inline int meet_params(const Pt& p1, const Pt& p2, const Pt& q1, const Pt& q2, double t[2]) {
    if (!segments_meet(p1, p2, q1, q2)) return 0;
    const double dx = p2.x - p1.x, dy = p2.y - p1.y;
    const double len2 = dx * dx + dy * dy;
    const int a = orientation(p1.x, p1.y, p2.x, p2.y, q1.x, q1.y);
    const int b = orientation(p1.x, p1.y, p2.x, p2.y, q2.x, q2.y);
    if (a == 0 && b == 0) {                    // collinear overlap
        const double t0 = meet_param_of(p1, dx, dy, len2, q1), t1 = meet_param_of(p1, dx, dy, len2, q2);
        t[0] = t0 > t1 ? t1 : t0;
        t[1] = t0 > t1 ? t0 : t1;
        return 2;
    }
    if (a == 0) { t[0] = meet_param_of(p1, dx, dy, len2, q1); return 1; }
    if (b == 0) { t[0] = meet_param_of(p1, dx, dy, len2, q2); return 1; }
    // proper or end-of-p touch: solve with the cross products
    const double ex = q2.x - q1.x, ey = q2.y - q1.y;
    const double den = dx * ey - dy * ex;
    const double v = den != 0 ? ((q1.x - p1.x) * ey - (q1.y - p1.y) * ex) / den : 0.0;
    t[0] = v < 0 ? 0.0 : (v > 1 ? 1.0 : v);
    return 1;
}

// midpoint of the piece (t0, t1) of segment (a, b): the point whose membership stands for the piece
TD_GEOM_HD inline Pt piece_midpoint(const Pt& a, const Pt& b, double t0, double t1) {
    const double tm = 0.5 * (t0 + t1);
    return {a.x + tm * (b.x - a.x), a.y + tm * (b.y - a.y)};
}

// one edge (a, b) of the (small) query ring against point p, as edge_point_rule without its early outs: 1 on it, 2 crossing
TD_GEOM_HD inline int query_edge_rule(const Pt& a, const Pt& b, const Pt& p) {
    const int o = orientation(a.x, a.y, b.x, b.y, p.x, p.y);
    if (o == 0 && env_has(a, b, p)) return 1;
    if ((a.y <= p.y) != (b.y <= p.y)) {
        const bool up = a.y <= p.y;
        if ((up && o > 0) || (!up && o < 0)) return 2;
    }
    return 0;
}

// closed point-in-ring for the (small) query ring: 0 outside, 1 inside, 2 on the boundary
TD_GEOM_HD inline int point_in_query(const Pt* q, int n, const Pt& p) {
    bool in = false;
    for (int i = 0; i + 1 < n; ++i) {
        const int c = query_edge_rule(q[i], q[i + 1], p);
        if (c == 1) return 2;
        if (c == 2) in = !in;
    }
    return in ? 1 : 0;
}

// y-bin of the edge index: bins of equal height from y0, the ends clamped
TD_GEOM_HD inline int relate_bin_of(double y, double y0, double inv_h, int nb) {
    const double f = (y - y0) * inv_h;
    if (!(f > 0)) return 0;
    return f >= nb ? nb - 1 : (int)f;
}

}  // namespace tdgeom
