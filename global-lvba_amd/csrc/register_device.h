// register_device.h -- point-to-plane registration of a scan against the voxel plane map (lvba_register_*): the per-point
// rule and the per-job Gauss-Newton step.  Also compiles as plain C++ (tests/register_check.cpp).  All arithmetic is fp64; the
// including file is built without floating-point contraction (the inlier gate is a discrete decision on a residual).
//   A job is a cloud of body-frame points p (fp32, promoted once) and a pose T = (R row-major | t).  Per point
//     w = (R00 px + R01 py) + R02 pz + tx, ...                         the world point (pose_apply, scan_points.h)
//     (n, d)                                                            its plane (voxel_lookup.h), if any
//     r = (n0 w0 + n1 w1) + n2 w2 + d                                   inlier iff a plane was found and |r| <= max_distance
//     J = [ p x (R^T n) ; n ]                                           d r / d(theta, t) under R <- R Exp(theta), t <- t + delta
//     s = r^2, rho = loss(s):  H += rho' J J^T, g += rho' J r, cost += rho          (first-order IRLS; no loss: rho = s, rho' = 1)
//   REG_NS sums per job: the upper triangle of H row by row (21), g (6), the cost, the inlier count (as a double: exact).
//   The step: too few inliers | degenerate (smallest eigenvalue of H / inliers below min_eigenvalue, or a pivot of the LDL^T of H
//   that is not positive) | delta = -H^-1 g, converged (|dtheta| <= tol_rot and |dt| <= tol_pos; the step is not applied) |
//   retract and continue.
#pragma once
#include <math.h>
#include <stdint.h>
#include "visual_loss.h"
#include "prior_device.h"
#include "scan_points.h"

namespace lvba {

constexpr int REG_NS = 29;                          // sums per job
constexpr int REG_G0 = 21, REG_COST = 27, REG_CNT = 28;
constexpr int REG_WS = 36 + 6 + 6;                  // reg_step's workspace: A (6 x 6), two vectors
// job states (results: the LVBA_REG_* values of include/lvba_hip.h; RUNNING is internal)
enum { REG_CONVERGED = 0, REG_MAX_ITERATIONS = 1, REG_TOO_FEW = 2, REG_DEGENERATE = 3, REG_RUNNING = -1 };

struct RegParams { // lvba_register_opts on the device
    double max_distance, min_eigenvalue, tol_rot, tol_pos, loss_scale;
    int64_t min_inliers;
    int32_t loss_kind;
};

// pose_apply (scan_points.h) under the name tests/register_check.cpp binds; new code calls pose_apply
LVBA_HD void reg_world(const double *T, const double p[3], double w[3]) { pose_apply(T, p[0], p[1], p[2], w); }

LVBA_HD double reg_residual(const double w[3], const double pl[4]) { return (pl[0] * w[0] + pl[1] * w[1]) + pl[2] * w[2] + pl[3]; }

// One associated point into the sums s[REG_NS] (registers on the device: every index is a constant after unrolling).
// Returns whether it is an inlier.
LVBA_HD bool reg_point(const double *T, const double p[3], const double w[3], const double pl[4], const RegParams &o, double *s)
{
    const double r = reg_residual(w, pl);
    if (!(fabs(r) <= o.max_distance)) return false;
    const double u0 = (T[0] * pl[0] + T[3] * pl[1]) + T[6] * pl[2]; // R^T n
    const double u1 = (T[1] * pl[0] + T[4] * pl[1]) + T[7] * pl[2];
    const double u2 = (T[2] * pl[0] + T[5] * pl[1]) + T[8] * pl[2];
    const double J[6] = {p[1] * u2 - p[2] * u1, p[2] * u0 - p[0] * u2, p[0] * u1 - p[1] * u0, pl[0], pl[1], pl[2]};
    double rho[3];
    loss_eval(o.loss_kind, o.loss_scale, r * r, rho);
    const double wt = rho[1];
    int k = 0;
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 6; ++a) {
        const double wa = wt * J[a];
LVBA_PRIOR_UNROLL
        for (int b = a; b < 6; ++b) s[k++] += wa * J[b];
        s[REG_G0 + a] += wa * r;
    }
    s[REG_COST] += rho[0];
    s[REG_CNT] += 1.0;
    return true;
}

// Eigenvalues of the symmetric n x n matrix A (row-major, destroyed; the diagonal holds them on return, unsorted) by cyclic
// Jacobi: the rotation of balm_math.h's eig3, swept over all pairs (p, q) in row order.  Returns the smallest.  A lives in
// memory the caller provides (LDS on the device): the indices are run-time values.
LVBA_HD double reg_jacobi_min(double *A, int n)
{
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += fabs(A[n * p + q]);
        if (off == 0.0) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[n * p + q];
                if (apq == 0.0) continue;
                const double app = A[n * p + p], aqq = A[n * q + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                A[n * p + p] = app - t * apq;
                A[n * q + q] = aqq + t * apq;
                A[n * p + q] = A[n * q + p] = 0.0;
                for (int r = 0; r < n; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = A[n * r + p], arq = A[n * r + q];
                    const double np_ = c * arp - sn * arq, nq_ = sn * arp + c * arq;
                    A[n * r + p] = A[n * p + r] = np_;
                    A[n * r + q] = A[n * q + r] = nq_;
                }
            }
    }
    double m = A[0];
    for (int p = 1; p < n; ++p) m = fmin(m, A[n * p + p]);
    return m;
}

// x = A^-1 b by LDL^T without pivoting (A symmetric n x n row-major, destroyed; b overwritten by x).  False: a pivot that is
// not positive (or not finite).
LVBA_HD bool reg_ldlt_solve(double *A, double *b, int n)
{
    for (int j = 0; j < n; ++j) {
        double d = A[n * j + j];
        for (int k = 0; k < j; ++k) d -= A[n * j + k] * A[n * j + k] * A[n * k + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        A[n * j + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double v = A[n * i + j];
            for (int k = 0; k < j; ++k) v -= A[n * i + k] * A[n * j + k] * A[n * k + k];
            A[n * i + j] = v / d;
        }
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k) b[i] -= A[n * i + k] * b[k];
    for (int i = 0; i < n; ++i) b[i] /= A[n * i + i];
    for (int i = n - 1; i >= 0; --i)
        for (int k = i + 1; k < n; ++k) b[i] -= A[n * k + i] * b[k];
    return true;
}

// The full symmetric matrix of the 21 upper-triangle sums, times scale
LVBA_HD void reg_expand(const double *s, double scale, double *A)
{
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[6 * a + b] = A[6 * b + a] = s[k] * scale; ++k; }
}

// One Gauss-Newton step of a job from its sums s[REG_NS].  ws: REG_WS doubles of workspace.  Returns the job's state; on
// REG_RUNNING the pose T [12] has been retracted.  *min_eig, *rmse: of this linearisation (0 when there are too few inliers).
LVBA_HD int reg_step(const double *s, const RegParams &o, double *T, double *ws, double *min_eig, double *rmse)
{
    *min_eig = 0.0; *rmse = 0.0;
    const double cnt = s[REG_CNT];
    if (cnt < (double)(o.min_inliers > 1 ? o.min_inliers : 1)) return REG_TOO_FEW;
    *rmse = sqrt(s[REG_COST] / cnt);
    double *A = ws, *x = ws + 36;
    reg_expand(s, 1.0 / cnt, A);
    *min_eig = reg_jacobi_min(A, 6);
    if (!(*min_eig >= o.min_eigenvalue)) return REG_DEGENERATE;
    reg_expand(s, 1.0, A);
    for (int a = 0; a < 6; ++a) x[a] = -s[REG_G0 + a];
    if (!reg_ldlt_solve(A, x, 6)) return REG_DEGENERATE;
    const double dth = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), dt = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    if (!(isfinite(dth) && isfinite(dt))) return REG_DEGENERATE;
    if (dth <= o.tol_rot && dt <= o.tol_pos) return REG_CONVERGED;
    const double w3[3] = {x[0], x[1], x[2]};
    double E[9], Rn[9];
    so3_exp(w3, E);
    m3_mul(T, E, Rn);
    for (int a = 0; a < 9; ++a) T[a] = Rn[a];
    T[9] += x[3]; T[10] += x[4]; T[11] += x[5];
    return REG_RUNNING;
}

} // namespace lvba
