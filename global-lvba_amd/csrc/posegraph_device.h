// posegraph_device.h -- per-edge arithmetic of the pose-graph relaxation (lvba_posegraph_relax; pose_graph.hip; the problem and the
// LM rule are in include/lvba_hip.h).  Also compiles as plain C++ (tests/posegraph_check.cpp).
//   An edge is a prior of prior_device.h (RELATIVE: odometry steps and closures; POSE: the anchor) with the record layout of the
//   prior tables (meas | oi | oj | L).  The residual, the whitened blocks (prior_eval) and the lin record (prior_record, layout
//   PL_*) are prior_device.h's; what is added here is the odometry measurement Z0_i = X_i^-1 X_{i+1}, and the robust weight of a closure: with e = L r, s = |e|^2,
//   an edge under a loss rho (visual_loss.h) costs 1/2 rho(s) and its J^T e and 6 x 6 products carry the factor rho'(s) -- applied
//   as sqrt(rho') on e and on the whitened blocks before the products are formed (Ceres' corrector, scaling branch: the rho'' term
//   is left out as everywhere in this project).
#pragma once
#include "prior_device.h"
#include "visual_loss.h"

namespace lvba {

// Z = X_i^-1 X_j (poses as R row-major | p)
LVBA_HD void pg_relative(const double *Xi, const double *Xj, double *Z)
{
    m3_tmul(Xi, Xj, Z);
    const double d[3] = {Xj[9] - Xi[9], Xj[10] - Xi[10], Xj[11] - Xi[11]};
    m3_tvec(Xi, d, Z + 9);
}

// The record of an odometry step between input poses Xi, Xj: meas = Z0, identity offsets, L = diag(1/sigma_rot x 3, 1/sigma_pos x 3)
LVBA_HD void pg_odometry_record(const double *Xi, const double *Xj, double inv_sigma_rot, double inv_sigma_pos, double *meas, double *oi,
                                double *oj, double *L)
{
    pg_relative(Xi, Xj, meas);
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 12; ++a) oi[a] = oj[a] = (a == 0 || a == 4 || a == 8) ? 1.0 : 0.0;
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 36; ++a) L[a] = 0.0;
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 6; ++a) L[7 * a] = a < 3 ? inv_sigma_rot : inv_sigma_pos;
}

// cost 1/2 rho(|e|^2) of an edge and its weight rho' (loss_kind 0: 1/2 |e|^2 and 1)
LVBA_HD double pg_edge_cost(int kind, const double *meas, const double *oi, const double *oj, const double *L, const double *Ti, const double *Tj,
                            int loss_kind, double loss_scale, double *weight)
{
    double e[6];
    const double half = prior_eval(kind, meas, oi, oj, L, Ti, Tj, e, false, nullptr, nullptr);
    if (loss_kind == VLOSS_TRIVIAL) { *weight = 1.0; return half; }
    double rho[3];
    loss_eval(loss_kind, loss_scale, 2.0 * half, rho);
    *weight = rho[1];
    return 0.5 * rho[0];
}

// The weighted lin record o [PL_LIN] of an edge (kind is a constant at each call site: every array stays in registers); returns the
// cost, *weight = rho'.  Between prior_eval and prior_record, e and the whitened blocks take the factor sqrt(rho').
LVBA_HD double pg_edge_lin(const int kind, const double *meas, const double *oi, const double *oj, const double *L, const double *Ti,
                           const double *Tj, bool flip, int loss_kind, double loss_scale, double *o, double *weight)
{
    double e[6], Wi[36], Wj[36];
    double cost = prior_eval(kind, meas, oi, oj, L, Ti, Tj, e, true, Wi, Wj);
    *weight = 1.0;
    if (loss_kind != VLOSS_TRIVIAL) {
        double rho[3];
        loss_eval(loss_kind, loss_scale, 2.0 * cost, rho);
        cost = 0.5 * rho[0];
        *weight = rho[1];
        const double sw = sqrt(rho[1]);
LVBA_PRIOR_UNROLL
        for (int a = 0; a < 6; ++a) e[a] *= sw;
LVBA_PRIOR_UNROLL
        for (int a = 0; a < 36; ++a) Wi[a] *= sw;
        if (kind == PRIOR_RELATIVE) {
LVBA_PRIOR_UNROLL
            for (int a = 0; a < 36; ++a) Wj[a] *= sw;
        }
    }
    prior_record(kind, e, Wi, Wj, flip, o);
    return cost;
}

} // namespace lvba
