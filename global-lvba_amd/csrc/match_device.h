// match_device.h -- scalar pieces of the descriptor matcher (match.hip; the rule is in include/lvba_hip.h):
// the running top two of a row, their merge, the epipolar gate, the depth gate and the fp64 decision.  Host/device-neutral, like
// tracks_device.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include "tracks_device.h"
#include "fusion_device.h"

namespace lvba {

constexpr int MATCH_DIM = 128;                    // bytes per descriptor
constexpr int32_t MATCH_NONE = INT32_MIN;         // "no column yet": below every biased score
// sum a b = sum a'b' + 128 (sum a' + sum b') + 128 * 128 * 128 with a' = a - 128: the last term
constexpr int32_t MATCH_BIAS_CONST = 128 * 128 * 128;
constexpr double MATCH_SCORE_SCALE = 262144.0;    // 512^2
constexpr double MATCH_BASELINE_REL2 = 1e-20;     // |t_ab|^2 <= this (|t_a|^2 + |t_b|^2): no epipolar geometry
enum MatchMode : int { MATCH_UNGUIDED = 0, MATCH_EPIPOLAR = 1, MATCH_DEPTH = 2 }; // lvba_match_opts::guided

// Running (s1, best, s2) of one row over the columns one lane sees, in ascending column order: a strict > keeps the lowest column
// of a tie.  The scores are biased by a per-row constant, which no comparison within a row sees.
struct MatchTop { int32_t s1, best, s2; };

LVBA_TRK_FN MatchTop match_top_none() { MatchTop t; t.s1 = MATCH_NONE; t.best = -1; t.s2 = MATCH_NONE; return t; }

LVBA_TRK_FN void match_top_update(MatchTop &t, int32_t v, int32_t col)
{
    const int32_t lo = v < t.s1 ? v : t.s1;       // s2 <= s1 always: the median of (v, s1, s2)
    t.s2 = t.s2 > lo ? t.s2 : lo;
    t.best = v > t.s1 ? col : t.best;
    t.s1 = v > t.s1 ? v : t.s1;
}

// the top two of the union of two disjoint column sets
LVBA_TRK_FN MatchTop match_top_merge(const MatchTop &a, const MatchTop &b)
{
    const bool a_wins = a.s1 > b.s1 || (a.s1 == b.s1 && (uint32_t)a.best < (uint32_t)b.best); // -1 (none) loses every tie
    MatchTop t;
    t.s1 = a_wins ? a.s1 : b.s1;
    t.best = a_wins ? a.best : b.best;
    const int32_t other = a_wins ? b.s1 : a.s1, own = a_wins ? a.s2 : b.s2;
    t.s2 = own > other ? own : other;
    return t;
}

// Epipolar gate.  "lo" is the image of the pair with the smaller index, "hi" the other; E maps lo to hi.  Both orientations of a
// pair evaluate these same expressions on the same operands, so the decision for (r, c) and for (c, r) is one bit.
struct MatchLine { double l0, l1, l2, n; };

LVBA_TRK_FN MatchLine match_line_lo(const double *E, double x, double y)   // l = E x, n = l0^2 + l1^2
{
    MatchLine m;
    m.l0 = (E[0] * x + E[1] * y) + E[2];
    m.l1 = (E[3] * x + E[4] * y) + E[5];
    m.l2 = (E[6] * x + E[7] * y) + E[8];
    m.n = m.l0 * m.l0 + m.l1 * m.l1;
    return m;
}
LVBA_TRK_FN double match_norm_hi(const double *E, double x, double y)       // l' = E^T x, l'0^2 + l'1^2
{
    const double m0 = (E[0] * x + E[3] * y) + E[6];
    const double m1 = (E[1] * x + E[4] * y) + E[7];
    return m0 * m0 + m1 * m1;
}
// the gate's bound for max_px pixels in normalised units, squared: tau = 2 max_px / (fx + fy) (match.hip and verify.hip, on the host)
inline double match_tau2(double focal_sum, double max_px) { const double tau = (2.0 * max_px) / focal_sum; return tau * tau; }
LVBA_TRK_FN bool match_gate(const MatchLine &lo, double hx, double hy, double n_hi, double tau2)
{
    const double e = (hx * lo.l0 + hy * lo.l1) + lo.l2;
    return e * e <= tau2 * (lo.n + n_hi);          // false when a NaN (failed undistortion) is in it
}

// E of the ordered pair (lo, hi) from T_cam<-world of both; all zero when the centres coincide
LVBA_TRK_FN void match_essential(const double *Rlo, const double *tlo, const double *Rhi, const double *thi, double *E)
{
    double R[9], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Rhi[3 * i] * Rlo[3 * j] + Rhi[3 * i + 1] * Rlo[3 * j + 1]) + Rhi[3 * i + 2] * Rlo[3 * j + 2];
    for (int i = 0; i < 3; ++i) t[i] = thi[i] - ((R[3 * i] * tlo[0] + R[3 * i + 1] * tlo[1]) + R[3 * i + 2] * tlo[2]);
    const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    const double ref = ((tlo[0] * tlo[0] + tlo[1] * tlo[1]) + tlo[2] * tlo[2]) + ((thi[0] * thi[0] + thi[1] * thi[1]) + thi[2] * thi[2]);
    if (tt <= MATCH_BASELINE_REL2 * ref) {
        for (int k = 0; k < 9; ++k) E[k] = 0.0;
        return;
    }
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}

// Depth gate.  A keypoint with a depth return is a 3-D point (match_lift: NaN where it has none); its prediction in another
// image is a pixel (match_predict): NaN for a keypoint without a point, +inf for a point that does not project ("nowhere"), so
// that neither needs a branch below -- a NaN or an infinite distance fails the comparison, and "has a point" is "the prediction
// is not NaN" (a projection that succeeds is finite).  Both orientations of a pair evaluate these same expressions on the same
// operands, so the decision for (r, c) and for (c, r) is one bit.
LVBA_TRK_FN void match_lift(const float *__restrict__ depth, int w, int h, float u, float v, double x, double y,
                            const double *__restrict__ R, const double *__restrict__ tc, double *__restrict__ X)
{
    double p[3];
    const bool ok = depth_world_point(depth, w, h, u, v, x, y, R, tc, p) && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    X[0] = ok ? p[0] : NAN; X[1] = ok ? p[1] : NAN; X[2] = ok ? p[2] : NAN;
}
LVBA_TRK_FN void match_predict(const TrkIntr &cam, const double *R, const double *t, const double *X, double &pu, double &pv)
{
    if (X[0] != X[0]) { pu = pv = NAN; return; }
    if (!trk_project(cam, R, t, X, pu, pv)) pu = pv = INFINITY;
}
struct MatchReproj { double u, v, pu, pv; };      // a keypoint's own pixel and its prediction in the other image of the pair
LVBA_TRK_FN bool match_reproj_near(double u, double v, double pu, double pv, double rho2)   // d^2 <= rho^2
{
    const double du = u - pu, dv = v - pv;
    return du * du + dv * dv <= rho2;
}
LVBA_TRK_FN bool match_depth_gate(const MatchReproj &p, const MatchReproj &q, double rho2)
{
    const bool hp = p.pu == p.pu, hq = q.pu == q.pu;
    const bool near_q = match_reproj_near(q.u, q.v, p.pu, p.pv, rho2), near_p = match_reproj_near(p.u, p.v, q.pu, q.pv, rho2);
    return (hp | hq) & (near_q | !hp) & (near_p | !hq);
}

LVBA_TRK_FN double match_distance(int32_t s)
{
    const double c = (double)s / MATCH_SCORE_SCALE;
    return acos(c < 1.0 ? c : 1.0);
}
// the one-sided clauses of a match (the mutual clause is the caller's)
LVBA_TRK_FN bool match_accept(int32_t best, int32_t s1, int32_t s2, double max_distance, double max_ratio)
{
    if (best < 0) return false;
    const double d1 = match_distance(s1), d2 = match_distance(s2);
    return d1 < max_distance && d1 < max_ratio * d2;
}

} // namespace lvba
