// calib_device.h -- LiDAR-camera extrinsic refinement from depth-lifted matches (lvba_calib_*; the rule is in include/lvba_hip.h,
// DESIGN.md §10o): the pair transform, the per-record rule, the partition of the records over workgroups and the per-job step.
// Also compiles as plain C++ (tests/calib_check.cpp).  All arithmetic is fp64, every expression rounds in the order written here,
// and the including file is built without floating-point contraction: a record's residual, Jacobian and weight are the same bits
// under g++, numpy and gfx950 (+, -, *, / and sqrt only with the trivial and the Huber loss).  The sums are a tree on the device
// and are held to the summation bound instead.
//   (R, t) = T_cam<-imu, the unknown.  A record is a keypoint (x, y) (undistorted, normalised) of image a and the point Xb its match
//   in image b was lifted to, in b's camera frame; A = (R_ab | p_ab) = T_imu_a<-imu_b of the record's pair.
//     d = Xb - t,  q = R^T d,  w = R_ab q + p_ab,  Xc = R w + t                 the point in a's camera frame: X A X^-1 Xb
//     iz = 1 / Xc_z, px = Xc_x iz, py = Xc_y iz,  r = (fx (px - x), fy (py - y))  (resect_accumulate's form)
//     counted iff Xc_z > 1e-12 and, with a gate, r0 r0 + r1 r1 <= max_error_px max_error_px
//   Left perturbation R <- (I + [om]x) R, t <- t + om x t + up; with M = R R_ab R^T
//     dXc/dom = -[Xc]x + M [Xb]x,  dXc/dup = I - M
//   and with g the gradient of a residual component by Xc and h = M^T g = R (R_ab^T (R^T g)) its row of the Jacobian is
//     J_om = Xc x g + h x Xb,  J_up = g - h                                      (M itself is never formed)
//   s = |r|^2, rho = loss_eval(s): weight rho', H += rho' J^T J, g += rho' J^T r, cost += rho / 2.
#pragma once
#include <math.h>
#include <stdint.h>
#include "visual_loss.h"
#include "tracks_device.h"
#include "resect_device.h"

namespace lvba {

constexpr int CAL_NS = 31;                          // sums per job: H upper triangle by row (21), g (6), cost, count, sum |r|^2, sum rho'
constexpr int CAL_G0 = 21, CAL_COST = 27, CAL_CNT = 28, CAL_SSQ = 29, CAL_SW = 30;
constexpr int CAL_WS = 36 + 36 + 6 + 6;             // cal_step's workspace: A, V (6 x 6), the eigenvalues, the step
// the partition of n records over the linearisation's workgroups: lane l of workgroup b takes the records
// b * CAL_BLOCK + l + k * nb * CAL_BLOCK, k = 0, 1, ...
constexpr int CAL_BLOCK = 256;                      // lanes of a linearisation workgroup
constexpr int CAL_RUN = 8;                          // records per lane up to CAL_MAX_BLOCKS workgroups
constexpr int CAL_MAX_BLOCKS = 512;                 // two workgroups per compute unit of a 256-unit device
constexpr double CAL_MIN_DEPTH = RESECT_MIN_DEPTH;  // projectCameraToPixel's cheirality bound
// H carries information only where its largest eigenvalue is above this times count (fx^2 + fy^2): a unit of rotation moves a pixel
// by about a focal length, so this is a sensitivity of 1e-10 px per pixel of full sensitivity -- far above the square of the
// Jacobian's rounding (1e-32), which is all that H holds where the body never moves, far below anything a trajectory gives
constexpr double CAL_EIG_FLOOR = 1e-20;
// job states (the LVBA_CALIB_* values of include/lvba_hip.h; RUNNING is internal)
enum { CAL_CONVERGED = 0, CAL_MAX_ITERATIONS = 1, CAL_TOO_FEW = 2, CAL_DEGENERATE = 3, CAL_RUNNING = -1 };

struct CalParams { // lvba_calib_opts and the focal lengths on the device
    double fx, fy, max_error_px, loss_scale, min_eig_ratio, eps_rot, eps_trans;
    int64_t min_records;
    int32_t loss_kind;
};

struct CalResult { // a job's state and what it reports, of its last linearisation
    int32_t status, iterations, n_held, pad;
    int64_t n_used;
    double rmse, cost;
    double eig[6];      // ascending
    double vec[36];     // row k: the unit eigenvector of eig[k], order (om, up)
};

// the number of workgroups n records are summed by: a function of n alone
LVBA_TRK_FN int cal_blocks(int64_t n)
{
    const int64_t nb = (n + (int64_t)CAL_BLOCK * CAL_RUN - 1) / ((int64_t)CAL_BLOCK * CAL_RUN);
    return (int)(nb < 1 ? 1 : nb > CAL_MAX_BLOCKS ? CAL_MAX_BLOCKS : nb);
}

// A [12] = (R_ab row-major | p_ab) of the body poses Ta, Tb = T_world<-imu [12]: R_ab = Rwi_a^T Rwi_b, p_ab = Rwi_a^T (P_b - P_a)
LVBA_TRK_FN void cal_pair(const double *Ta, const double *Tb, double *A)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = (Ta[i] * Tb[j] + Ta[3 + i] * Tb[3 + j]) + Ta[6 + i] * Tb[6 + j];
    const double d0 = Tb[9] - Ta[9], d1 = Tb[10] - Ta[10], d2 = Tb[11] - Ta[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) A[9 + i] = (Ta[i] * d0 + Ta[3 + i] * d1) + Ta[6 + i] * d2;
}

// the record's target coordinates: (x, y) of trk_undistort, NaN where it fails or where Xb is not finite (UNUSABLE: never counted)
LVBA_TRK_FN void cal_target(const TrkIntr &cam, float u, float v, const double *Xb, double &x, double &y)
{
    if (!(isfinite(Xb[0]) && isfinite(Xb[1]) && isfinite(Xb[2])) || !trk_undistort(cam, (double)u, (double)v, x, y)) x = y = NAN;
}

// what cal_eval forms on its way and the time-offset column (calib_td_device.h) is made of: q = R^T (Xb - t), w = R_ab q + p_ab and
// a0, a1 = R^T g of the two residual components' gradients by Xc
struct CalMid { double q[3], w[3], a0[3], a1[3]; };

// One record at (R, t) with its pair's transform A: false where it does not count (unusable, at or behind the camera, outside the
// gate); else r [2], the two rows J0, J1 [6] of its Jacobian in the order (om, up), rho [3] of its loss and m, its intermediates.
LVBA_TRK_FN bool cal_eval_mid(const double *R, const double *t, const double *A, double x, double y, const double *Xb, const CalParams &o,
                              double *r, double *J0, double *J1, double *rho, CalMid &m)
{
    if (!(x == x && y == y)) return false;
    const double d0 = Xb[0] - t[0], d1 = Xb[1] - t[1], d2 = Xb[2] - t[2];
    const double q0 = (R[0] * d0 + R[3] * d1) + R[6] * d2, q1 = (R[1] * d0 + R[4] * d1) + R[7] * d2,
                 q2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
    const double w0 = ((A[0] * q0 + A[1] * q1) + A[2] * q2) + A[9], w1 = ((A[3] * q0 + A[4] * q1) + A[5] * q2) + A[10],
                 w2 = ((A[6] * q0 + A[7] * q1) + A[8] * q2) + A[11];
    const double cx = ((R[0] * w0 + R[1] * w1) + R[2] * w2) + t[0], cy = ((R[3] * w0 + R[4] * w1) + R[5] * w2) + t[1],
                 cz = ((R[6] * w0 + R[7] * w1) + R[8] * w2) + t[2];
    if (!(cz > CAL_MIN_DEPTH)) return false;
    const double iz = 1.0 / cz, px = cx * iz, py = cy * iz;
    r[0] = o.fx * (px - x); r[1] = o.fy * (py - y);
    const double s = r[0] * r[0] + r[1] * r[1];
    if (o.max_error_px > 0.0 && !(s <= o.max_error_px * o.max_error_px)) return false;
    const double gx = o.fx * iz, gy = o.fy * iz, gz0 = -(gx * px), gz1 = -(gy * py);
    // h = R (R_ab^T (R^T g)) of g0 = (gx, 0, gz0) and g1 = (0, gy, gz1)
    const double a00 = R[0] * gx + R[6] * gz0, a01 = R[1] * gx + R[7] * gz0, a02 = R[2] * gx + R[8] * gz0;
    const double a10 = R[3] * gy + R[6] * gz1, a11 = R[4] * gy + R[7] * gz1, a12 = R[5] * gy + R[8] * gz1;
    const double b00 = (A[0] * a00 + A[3] * a01) + A[6] * a02, b01 = (A[1] * a00 + A[4] * a01) + A[7] * a02,
                 b02 = (A[2] * a00 + A[5] * a01) + A[8] * a02;
    const double b10 = (A[0] * a10 + A[3] * a11) + A[6] * a12, b11 = (A[1] * a10 + A[4] * a11) + A[7] * a12,
                 b12 = (A[2] * a10 + A[5] * a11) + A[8] * a12;
    const double h00 = (R[0] * b00 + R[1] * b01) + R[2] * b02, h01 = (R[3] * b00 + R[4] * b01) + R[5] * b02,
                 h02 = (R[6] * b00 + R[7] * b01) + R[8] * b02;
    const double h10 = (R[0] * b10 + R[1] * b11) + R[2] * b12, h11 = (R[3] * b10 + R[4] * b11) + R[5] * b12,
                 h12 = (R[6] * b10 + R[7] * b11) + R[8] * b12;
    J0[0] = gz0 * cy + (h01 * Xb[2] - h02 * Xb[1]);
    J0[1] = (gx * cz - gz0 * cx) + (h02 * Xb[0] - h00 * Xb[2]);
    J0[2] = -(gx * cy) + (h00 * Xb[1] - h01 * Xb[0]);
    J0[3] = gx - h00; J0[4] = -h01; J0[5] = gz0 - h02;
    J1[0] = (gz1 * cy - gy * cz) + (h11 * Xb[2] - h12 * Xb[1]);
    J1[1] = -(gz1 * cx) + (h12 * Xb[0] - h10 * Xb[2]);
    J1[2] = gy * cx + (h10 * Xb[1] - h11 * Xb[0]);
    J1[3] = -h10; J1[4] = gy - h11; J1[5] = gz1 - h12;
    loss_eval(o.loss_kind, o.loss_scale, s, rho);
    m.q[0] = q0; m.q[1] = q1; m.q[2] = q2; m.w[0] = w0; m.w[1] = w1; m.w[2] = w2;
    m.a0[0] = a00; m.a0[1] = a01; m.a0[2] = a02; m.a1[0] = a10; m.a1[1] = a11; m.a1[2] = a12;
    return true;
}

// cal_eval_mid without the intermediates
LVBA_TRK_FN bool cal_eval(const double *R, const double *t, const double *A, double x, double y, const double *Xb, const CalParams &o,
                          double *r, double *J0, double *J1, double *rho)
{
    CalMid m;
    return cal_eval_mid(R, t, A, x, y, Xb, o, r, J0, J1, rho, m);
}

// a counted record's terms into the sums s [CAL_NS] (registers on the device: every index is a constant after unrolling)
LVBA_TRK_FN void cal_accumulate(const double *r, const double *J0, const double *J1, const double *rho, double *s)
{
    const double wt = rho[1];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a; b < 6; ++b) s[k++] += wt * (J0[a] * J0[b] + J1[a] * J1[b]);
        s[CAL_G0 + a] += wt * (J0[a] * r[0] + J1[a] * r[1]);
    }
    s[CAL_COST] += 0.5 * rho[0];
    s[CAL_CNT] += 1.0;
    s[CAL_SSQ] += r[0] * r[0] + r[1] * r[1];
    s[CAL_SW] += wt;
}

LVBA_TRK_FN void cal_record(const double *R, const double *t, const double *A, double x, double y, const double *Xb, const CalParams &o,
                            double *s)
{
    double r[2], J0[6], J1[6], rho[3];
    if (cal_eval(R, t, A, x, y, Xb, o, r, J0, J1, rho)) cal_accumulate(r, J0, J1, rho, s);
}

// Eigen-decomposition of the symmetric n x n matrix A (row-major, destroyed: the diagonal holds the eigenvalues on return, unsorted)
// by cyclic Jacobi -- reg_jacobi_min's sweep (register_device.h), the rotations also applied to V, which returns with the
// eigenvector of A[k][k] in its column k.  A and V live in memory the caller provides (LDS on the device).
LVBA_TRK_FN void cal_jacobi(double *A, double *V, int n)
{
    for (int p = 0; p < n; ++p)
        for (int q = 0; q < n; ++q) V[n * p + q] = p == q ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += fabs(A[n * p + q]);
        if (!(off > 0.0)) break;   // also when a NaN is in it
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[n * p + q];
                if (apq == 0.0) continue;
                const double app = A[n * p + p], aqq = A[n * q + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                A[n * p + p] = app - tt * apq;
                A[n * q + q] = aqq + tt * apq;
                A[n * p + q] = A[n * q + p] = 0.0;
                for (int r = 0; r < n; ++r) {
                    const double vp = V[n * r + p], vq = V[n * r + q];
                    V[n * r + p] = c * vp - sn * vq;
                    V[n * r + q] = sn * vp + c * vq;
                    if (r == p || r == q) continue;
                    const double arp = A[n * r + p], arq = A[n * r + q];
                    const double np_ = c * arp - sn * arq, nq_ = sn * arp + c * arq;
                    A[n * r + p] = A[n * p + r] = np_;
                    A[n * r + q] = A[n * q + r] = nq_;
                }
            }
    }
}

// the full symmetric n x n matrix of the n (n + 1) / 2 upper-triangle sums
LVBA_TRK_FN void cal_expand_n(const double *s, double *A, int n)
{
    int k = 0;
    for (int a = 0; a < n; ++a)
        for (int b = a; b < n; ++b) { A[n * a + b] = A[n * b + a] = s[k]; ++k; }
}

LVBA_TRK_FN void cal_expand(const double *s, double *A) { cal_expand_n(s, A, 6); }

constexpr int CAL_MAX_N = 7;                        // the largest system cal_free_step takes (calib_td_device.h's)

// The eigen-decomposition, the held set and the step of an n-parameter job from its upper-triangle sums H and its gradient g.
// ws: 2 n n + 2 n doubles (A, V, the eigenvalues, the step).  Fills eig [n] ascending -- the lower index first of a tie --, vec
// [n][n] (row k the unit vector of eig[k]) and n_held, and returns the step d [n] = -sum over the free k of v_k (v_k . g) / eig[k],
// the sum in ascending k -- or nullptr (DEGENERATE): the largest eigenvalue is not above floor, or every direction is held (n_held
// = n either way).  Direction k is HELD where not eig[k] > min_eig_ratio * eig_max.
LVBA_TRK_FN const double *cal_free_step(int n, const double *H, const double *g, double min_eig_ratio, double floor, double *ws,
                                        double *eig, double *vec, int32_t &n_held)
{
    double *A = ws, *V = ws + n * n, *lam = ws + 2 * n * n, *d = lam + n;
    cal_expand_n(H, A, n);
    cal_jacobi(A, V, n);
    int order[CAL_MAX_N];
    for (int k = 0; k < n; ++k) {   // insertion sort by (eigenvalue, index)
        const double v = A[(n + 1) * k];
        int j = k;
        while (j > 0 && A[(n + 1) * order[j - 1]] > v) { order[j] = order[j - 1]; --j; }
        order[j] = k;
    }
    for (int k = 0; k < n; ++k) {
        lam[k] = eig[k] = A[(n + 1) * order[k]];
        for (int a = 0; a < n; ++a) vec[n * k + a] = V[n * a + order[k]];
    }
    double top = lam[0];
    for (int k = 1; k < n; ++k) top = lam[k] > top ? lam[k] : top;
    if (!(top > floor)) { n_held = n; return nullptr; }
    const double bound = min_eig_ratio * top;
    for (int a = 0; a < n; ++a) d[a] = 0.0;
    int held = 0;
    for (int k = 0; k < n; ++k) {
        if (!(lam[k] > bound)) { ++held; continue; }
        const double *v = vec + n * k;
        double vg = 0.0;
        for (int a = 0; a < n; ++a) vg += v[a] * g[a];
        const double c = vg / lam[k];
        for (int a = 0; a < n; ++a) d[a] -= v[a] * c;
    }
    n_held = held;
    return held == n ? nullptr : d;
}

// R <- (I + [om]x) R through a unit quaternion, t <- t + om x t + up (resect_step's retraction), d = (om, up)
LVBA_TRK_FN void cal_retract(const double *d, double *R, double *t)
{
    double Rn[9];
    for (int c = 0; c < 3; ++c) {
        Rn[c] = R[c] + (d[1] * R[6 + c] - d[2] * R[3 + c]);
        Rn[3 + c] = R[3 + c] + (d[2] * R[c] - d[0] * R[6 + c]);
        Rn[6 + c] = R[6 + c] + (d[0] * R[3 + c] - d[1] * R[c]);
    }
    const double tn[3] = {t[0] + (d[1] * t[2] - d[2] * t[1]) + d[3], t[1] + (d[2] * t[0] - d[0] * t[2]) + d[4],
                          t[2] + (d[0] * t[1] - d[1] * t[0]) + d[5]};
    resect_orthonormalise(Rn);
    for (int e = 0; e < 9; ++e) R[e] = Rn[e];
    t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
}

// The step of a job from its sums s [CAL_NS] at (R, t).  ws: CAL_WS doubles of workspace.  Fills out (n_used, rmse, cost, the
// eigenvalues ascending -- the lower index first of a tie --, their vectors, n_held) and returns the job's state:
//   TOO_FEW: count < min_records (eigenvalues and vectors zero, n_held 0).  DEGENERATE: the largest eigenvalue is not above
//   CAL_EIG_FLOOR count (fx^2 + fy^2) (not > 0 up to rounding), every direction is held, or the step is not finite.
//   Held set and step: cal_free_step.  CONVERGED where |om| <= eps_rot and |up| <=
//   eps_trans: the step is not applied, so what is reported is of the final extrinsic.  may_step false (the iteration limit is
//   reached): RUNNING becomes MAX_ITERATIONS without a step, for the same reason.  On RUNNING (R, t) has been retracted (cal_retract).
LVBA_TRK_FN int cal_step(const double *s, const CalParams &o, bool may_step, double *R, double *t, double *ws, CalResult &out)
{
    const double cnt = s[CAL_CNT];
    out.n_used = (int64_t)cnt;
    out.cost = s[CAL_COST];
    out.rmse = cnt > 0.0 ? sqrt(s[CAL_SSQ] / cnt) : 0.0;
    out.n_held = 0;
    for (int k = 0; k < 6; ++k) out.eig[k] = 0.0;
    for (int k = 0; k < 36; ++k) out.vec[k] = 0.0;
    if (cnt < (double)o.min_records) return CAL_TOO_FEW;
    const double *d = cal_free_step(6, s, s + CAL_G0, o.min_eig_ratio, CAL_EIG_FLOOR * cnt * (o.fx * o.fx + o.fy * o.fy), ws, out.eig,
                                    out.vec, out.n_held);
    if (!d) return CAL_DEGENERATE;
    const double dr = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), dt = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
    if (!(isfinite(dr) && isfinite(dt))) return CAL_DEGENERATE;
    if (dr <= o.eps_rot && dt <= o.eps_trans) return CAL_CONVERGED;
    if (!may_step) return CAL_MAX_ITERATIONS;
    cal_retract(d, R, t);
    return CAL_RUNNING;
}

} // namespace lvba
