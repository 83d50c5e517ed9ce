// calib_td_device.h -- the camera-LiDAR time offset as a seventh parameter of the extrinsic refinement (lvba_calib_*_td; the rule
// is in include/lvba_hip.h, DESIGN.md §10o "time offset"): the body pose of an image at an offset, the pair table's row, the
// record's seventh column, the 39 sums and the 7-parameter step.  On top of calib_device.h and under its terms: plain C++ too
// (tests/calib_td_check.cpp), fp64, every expression rounds in the order written, no contraction; +, -, *, / and sqrt only outside
// the loss, so a record's terms are the same bits under g++, numpy and gfx950.
//   The image stamped t was taken at t + td.  twist [6] = (om, v) of its body: om the body-frame angular velocity (rad/s), v the
//   world-frame linear velocity (m/s), constant around the image.  With th = td om, s = 1 + |th|^2 / 4:
//     C = I + ([th]x + [th]x^2 / 2) / s                 the Cayley map: an exact rotation about om by 2 atan(td |om| / 2)
//     R(td) = R C,  P(td) = P + td v
//   and dC/dtd = C [om']x with om' = om / (1 + td^2 |om|^2 / 4).  A pair's row E [21]: A(td) = cal_pair of the two shifted poses
//   (12), om'_a (3), om'_b (3), dv = R_a(td)^T (v_b - v_a) (3).  With cal_eval's q, w and a_k = R^T g_k:
//     dw = (R_ab (om'_b x q) - om'_a x w) + dv,  J_k[6] = (a_k0 dw0 + a_k1 dw1) + a_k2 dw2
#pragma once
#include "calib_device.h"

namespace lvba {

constexpr int CAL_TD_N = 7;                         // parameters: (om, up, td)
constexpr int CAL_TD_NS = 39;                       // sums per job: H upper triangle by row (28), g (7), cost, count, sum |r|^2, sum rho'
constexpr int CAL_TD_G0 = 28, CAL_TD_COST = 35, CAL_TD_CNT = 36, CAL_TD_SSQ = 37, CAL_TD_SW = 38;
constexpr int CAL_TD_ROW = 21;                      // doubles of a pair's row: A (12), om'_a, om'_b, dv
constexpr int CAL_TD_WS = 49 + 49 + 7 + 7;          // cal_td_step's workspace: cal_free_step's at n = 7
constexpr int CAL_TD_EXT = 13;                      // a job's unknowns: R row-major, t, td
constexpr int CAL_TD_OUT_OF_RANGE = 4;              // LVBA_CALIB_TD_OUT_OF_RANGE, beside calib_device.h's states
static_assert(CAL_TD_N <= CAL_MAX_N, "cal_free_step's order array");

struct CalTdParams { // lvba_calib_td_opts on the device
    CalParams cal;
    double eps_td, max_abs_td;
};

struct CalTdResult { // CalResult at seven parameters
    int32_t status, iterations, n_held, pad;
    int64_t n_used;
    double rmse, cost;
    double eig[7];      // ascending
    double vec[49];     // row k: the unit eigenvector of eig[k], order (om, up, td)
};

// T(td) [12] of the body pose T = T_world<-imu [12] and its twist [6]
LVBA_TRK_FN void cal_td_pose(const double *T, const double *twist, double td, double *out)
{
    const double th0 = td * twist[0], th1 = td * twist[1], th2 = td * twist[2];
    const double s = 1.0 + 0.25 * ((th0 * th0 + th1 * th1) + th2 * th2);
    // [th]x + [th]x^2 / 2 entry by entry: [th]x^2 = th th^T - |th|^2 I
    const double C[9] = {1.0 + (0.5 * -(th1 * th1 + th2 * th2)) / s, (-th2 + 0.5 * (th0 * th1)) / s, (th1 + 0.5 * (th0 * th2)) / s,
                         (th2 + 0.5 * (th0 * th1)) / s, 1.0 + (0.5 * -(th0 * th0 + th2 * th2)) / s, (-th0 + 0.5 * (th1 * th2)) / s,
                         (-th1 + 0.5 * (th0 * th2)) / s, (th0 + 0.5 * (th1 * th2)) / s, 1.0 + (0.5 * -(th0 * th0 + th1 * th1)) / s};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (T[3 * i] * C[j] + T[3 * i + 1] * C[3 + j]) + T[3 * i + 2] * C[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[9 + i] = T[9 + i] + td * twist[3 + i];
}

// om' [3] = om / (1 + td^2 |om|^2 / 4)
LVBA_TRK_FN void cal_td_rate(const double *twist, double td, double *out)
{
    const double den = 1.0 + 0.25 * ((td * td) * ((twist[0] * twist[0] + twist[1] * twist[1]) + twist[2] * twist[2]));
    out[0] = twist[0] / den; out[1] = twist[1] / den; out[2] = twist[2] / den;
}

// the row E [CAL_TD_ROW] of the pair (a, b) at td, from the two images' given poses and twists
LVBA_TRK_FN void cal_td_pair(const double *Ta, const double *Tb, const double *twa, const double *twb, double td, double *E)
{
    double Sa[12], Sb[12];
    cal_td_pose(Ta, twa, td, Sa);
    cal_td_pose(Tb, twb, td, Sb);
    cal_pair(Sa, Sb, E);
    cal_td_rate(twa, td, E + 12);
    cal_td_rate(twb, td, E + 15);
    const double e0 = twb[3] - twa[3], e1 = twb[4] - twa[4], e2 = twb[5] - twa[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) E[18 + i] = (Sa[i] * e0 + Sa[3 + i] * e1) + Sa[6 + i] * e2;
}

// cal_eval at A(td) = E [0 .. 11] with the seventh column: r [2], J0, J1 [7] in the order (om, up, td), rho [3]
LVBA_TRK_FN bool cal_td_eval(const double *R, const double *t, const double *E, double x, double y, const double *Xb, const CalParams &o,
                             double *r, double *J0, double *J1, double *rho)
{
    CalMid m;
    if (!cal_eval_mid(R, t, E, x, y, Xb, o, r, J0, J1, rho, m)) return false;
    const double *oa = E + 12, *ob = E + 15, *dv = E + 18;
    const double c0 = ob[1] * m.q[2] - ob[2] * m.q[1], c1 = ob[2] * m.q[0] - ob[0] * m.q[2], c2 = ob[0] * m.q[1] - ob[1] * m.q[0];
    const double e0 = oa[1] * m.w[2] - oa[2] * m.w[1], e1 = oa[2] * m.w[0] - oa[0] * m.w[2], e2 = oa[0] * m.w[1] - oa[1] * m.w[0];
    const double dw0 = (((E[0] * c0 + E[1] * c1) + E[2] * c2) - e0) + dv[0], dw1 = (((E[3] * c0 + E[4] * c1) + E[5] * c2) - e1) + dv[1],
                 dw2 = (((E[6] * c0 + E[7] * c1) + E[8] * c2) - e2) + dv[2];
    J0[6] = (m.a0[0] * dw0 + m.a0[1] * dw1) + m.a0[2] * dw2;
    J1[6] = (m.a1[0] * dw0 + m.a1[1] * dw1) + m.a1[2] * dw2;
    return true;
}

// a counted record's terms into the sums s [CAL_TD_NS] (registers on the device: every index is a constant after unrolling)
LVBA_TRK_FN void cal_td_accumulate(const double *r, const double *J0, const double *J1, const double *rho, double *s)
{
    const double wt = rho[1];
    int k = 0;
#pragma unroll
    for (int a = 0; a < CAL_TD_N; ++a) {
#pragma unroll
        for (int b = a; b < CAL_TD_N; ++b) s[k++] += wt * (J0[a] * J0[b] + J1[a] * J1[b]);
        s[CAL_TD_G0 + a] += wt * (J0[a] * r[0] + J1[a] * r[1]);
    }
    s[CAL_TD_COST] += 0.5 * rho[0];
    s[CAL_TD_CNT] += 1.0;
    s[CAL_TD_SSQ] += r[0] * r[0] + r[1] * r[1];
    s[CAL_TD_SW] += wt;
}

LVBA_TRK_FN void cal_td_record(const double *R, const double *t, const double *E, double x, double y, const double *Xb, const CalParams &o,
                               double *s)
{
    double r[2], J0[CAL_TD_N], J1[CAL_TD_N], rho[3];
    if (cal_td_eval(R, t, E, x, y, Xb, o, r, J0, J1, rho)) cal_td_accumulate(r, J0, J1, rho, s);
}

// cal_step at seven parameters, from the sums s [CAL_TD_NS] at x = (R, t, td) [CAL_TD_EXT].  ws: CAL_TD_WS doubles.  As cal_step,
// and: CONVERGED also needs |d[6]| <= eps_td; a step that would leave |td| > max_abs_td is not applied and the state is
// CAL_TD_OUT_OF_RANGE (the caller hands the job's start values back); on RUNNING td <- td + d[6] beside cal_retract.
LVBA_TRK_FN int cal_td_step(const double *s, const CalTdParams &o, bool may_step, double *x, double *ws, CalTdResult &out)
{
    const double cnt = s[CAL_TD_CNT];
    out.n_used = (int64_t)cnt;
    out.cost = s[CAL_TD_COST];
    out.rmse = cnt > 0.0 ? sqrt(s[CAL_TD_SSQ] / cnt) : 0.0;
    out.n_held = 0;
    for (int k = 0; k < 7; ++k) out.eig[k] = 0.0;
    for (int k = 0; k < 49; ++k) out.vec[k] = 0.0;
    if (cnt < (double)o.cal.min_records) return CAL_TOO_FEW;
    const double *d = cal_free_step(CAL_TD_N, s, s + CAL_TD_G0, o.cal.min_eig_ratio,
                                    CAL_EIG_FLOOR * cnt * (o.cal.fx * o.cal.fx + o.cal.fy * o.cal.fy), ws, out.eig, out.vec, out.n_held);
    if (!d) return CAL_DEGENERATE;
    const double dr = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), dt = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
    if (!(isfinite(dr) && isfinite(dt) && isfinite(d[6]))) return CAL_DEGENERATE;
    if (dr <= o.cal.eps_rot && dt <= o.cal.eps_trans && fabs(d[6]) <= o.eps_td) return CAL_CONVERGED;
    if (!may_step) return CAL_MAX_ITERATIONS;
    const double td = x[12] + d[6];
    if (fabs(td) > o.max_abs_td) return CAL_TD_OUT_OF_RANGE;
    cal_retract(d, x, x + 9);
    x[12] = td;
    return CAL_RUNNING;
}

} // namespace lvba
