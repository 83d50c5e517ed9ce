// visual_prior_device.h -- camera pose priors of the visual bundle adjustment (lvba_visual_set_priors).  Also compiles as plain
// C++ (tests/visual_prior_check.cpp).
//   A camera is (q, t) = T_cam<-world, q = [w,x,y,z] (normalised inside, like ceres::QuaternionRotatePoint).  The pose a prior
//   sees is the camera's pose in the world, T = T_world<-cam = (R(q)^T, -R(q)^T t); kinds, offsets, residual order and sqrt_info
//   are those of the LiDAR stage (prior_device.h, included: prior_raw / prior_whiten / prior_whiten_jac do the work).
//   prior_raw differentiates w.r.t. BALM's retraction of T, R <- R Exp(dphi), p <- p + dp.  The visual stage moves (q, t) by
//   EigenQuaternionManifold::Plus on the [w,x,y,z] memory (visual_math.h) and t additively, tangent d = [dq(3); dt(3)]; to first
//   order the ambient quaternion moves by P(q) dq (PlusJacobian, columns (dw, dv) below), the unit quaternion u = q/|q| by that
//   over |q| (the columns are tangent to the sphere), and R(u) <- Exp(w) R(u) with (0, w) = 2 du u^*, so
//        dphi = -w = G dq,   G[:, m] = -(2 / |q|^2) (w dv_m - dw_m v + v x dv_m)         (R^T <- R^T Exp(-w))
//        dp   = R^T [t]x dphi - R^T dt
//   vprior_pose gives T and that 6 x 6 chain matrix C (row-major): [dphi; dp] = C [dq; dt].
#pragma once
#include "prior_device.h"

namespace lvba {

// T (R row-major | p) = T_world<-cam of the camera (q, t); if jac, C (6 x 6 row-major) = d(BALM tangent of T) / d(visual tangent)
LVBA_HD void vprior_pose(const double *q, const double *t, double *T, bool jac, double *C)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double s = 2.0 / (w * w + x * x + y * y + z * z);
    // R(q / |q|), transposed into T
    T[0] = 1.0 - s * (y * y + z * z); T[3] = s * (x * y - w * z);       T[6] = s * (x * z + w * y);
    T[1] = s * (x * y + w * z);       T[4] = 1.0 - s * (x * x + z * z); T[7] = s * (y * z - w * x);
    T[2] = s * (x * z - w * y);       T[5] = s * (y * z + w * x);       T[8] = 1.0 - s * (x * x + y * y);
    double p[3];
    m3_vec(T, t, p);
    T[9] = -p[0]; T[10] = -p[1]; T[11] = -p[2];
    if (!jac) return;
    // PlusJacobian columns of the memory [w,x,y,z] read as Eigen [x,y,z,w]: (dw; dv) of tangent direction m
    const double dw[3] = {z, y, -x};
    const double dv[3][3] = {{-y, x, -w}, {z, -w, -x}, {w, z, -y}};
    double G[9], M[9], N[9];
LVBA_PRIOR_UNROLL
    for (int m = 0; m < 3; ++m) {
        const double *d = dv[m];
        G[m] = -s * (w * d[0] - dw[m] * x + (y * d[2] - z * d[1]));
        G[3 + m] = -s * (w * d[1] - dw[m] * y + (z * d[0] - x * d[2]));
        G[6 + m] = -s * (w * d[2] - dw[m] * z + (x * d[1] - y * d[0]));
    }
    m3_mul_hat(T, t, M); // R^T [t]x
    m3_mul(M, G, N);
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) {
            C[6 * r + c] = G[3 * r + c];
            C[6 * r + 3 + c] = 0.0;
            C[6 * (r + 3) + c] = N[3 * r + c];
            C[6 * (r + 3) + 3 + c] = -T[3 * r + c];
        }
}

// W = L J C (6 x 6 row-major): the whitened Jacobian block in the visual tangent
LVBA_HD void vprior_chain(int kind, const double *L, const double *J, const double *C, double *W)
{
    double JC[36];
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 6; ++a)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
LVBA_PRIOR_UNROLL
            for (int b = 0; b < 6; ++b) v += J[6 * a + b] * C[6 * b + c];
            JC[6 * a + c] = v;
        }
    prior_whiten_jac(kind, L, JC, W);
}

// One prior at the cameras (qi, ti), (qj, tj) (the second unused unless RELATIVE): e = L r (6; POSITION: e[3..5] = 0), returns
// 1/2 |e|^2; if jac, Wi / Wj = d e / d(visual tangent of camera i / j), row-major 6 x 6 (Wj: RELATIVE only).  meas, oi, oj as
// R row-major | t (offsets already resolved: the identity is written out), L row-major.
LVBA_HD double vprior_eval(int kind, const double *meas, const double *oi, const double *oj, const double *L, const double *qi,
                           const double *ti, const double *qj, const double *tj, double *e, bool jac, double *Wi, double *Wj)
{
    double Ti[12], Tj[12], Ci[36], Cj[36], r[6], Ji[36], Jj[36];
    vprior_pose(qi, ti, Ti, jac, Ci);
    if (kind == PRIOR_RELATIVE) vprior_pose(qj, tj, Tj, jac, Cj);
    prior_raw(kind, meas, Ti, oi, Tj, oj, r, jac, Ji, Jj);
    const double cost = prior_whiten(kind, L, r, e);
    if (jac) {
        vprior_chain(kind, L, Ji, Ci, Wi);
        if (kind == PRIOR_RELATIVE) vprior_chain(kind, L, Jj, Cj, Wj);
    }
    return cost;
}

} // namespace lvba
