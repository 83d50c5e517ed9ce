// resect_device.h -- scalar pieces of the camera resectioning (resect.hip; the rule is in include/lvba_hip.h): the
// correspondence record, the inlier test, the three-point minimal solver with its fourth-point choice, the Gauss-Newton refit on
// the six pose parameters and the re-orthonormalisation through a unit quaternion.  Host/device-neutral; the generator, the sampler,
// the rank and the status are ransac_device.h'.  The hypothesis stage uses +, -, *, / and sqrt only, in the order
// written here, and resect.hip is built without contraction: a hypothesis is the same bits on the host and on the device.  The
// refit's sums are taken in another order on the device (a tree) and it is held to a measured tolerance instead.
#pragma once
#include <math.h>
#include <stdint.h>
#include "ransac_device.h"

namespace lvba {

constexpr int RESECT_OK = RANSAC_OK, RESECT_TOO_FEW_MATCHES = RANSAC_TOO_FEW_MATCHES, RESECT_NO_MODEL = RANSAC_NO_MODEL,
              RESECT_TOO_FEW_INLIERS = RANSAC_TOO_FEW_INLIERS;
constexpr int RESECT_K = 4;                       // draws per hypothesis: three for the solver, one to choose among its solutions
constexpr int RESECT_REC = 5;                     // doubles per correspondence record: x, y, X0, X1, X2 (40 bytes; resect.hip says why)
constexpr double RESECT_MIN_DEPTH = 1e-12;        // projectCameraToPixel's cheirality bound
// |(X1 - X2) x (X1 - X3)|^2 <= this |X1 - X2|^2 |X1 - X3|^2 (sin^2 of the triangle's angle at X1): degenerate triangle
constexpr double RESECT_TRIANGLE_REL2 = 1e-12;
// the rank-2 form D0 splits into two real planes only where a diagonal entry of -adj(D0) is above this share of max|D0|^2
constexpr double RESECT_SPLIT_REL = 1e-14;
constexpr int RESECT_NEWTON = 16;                 // Newton steps on the cubic, all taken
constexpr int RESECT_POLISH = 3;                  // Gauss-Newton steps on the three depths
constexpr int RESECT_GN_STEPS = 4;                // Gauss-Newton steps on the pose per refinement round
constexpr int RESECT_NSUM = 28;                   // 21 entries of J^T J (upper triangle by row), 6 of J^T r, sum r^2

// ---- the record ------------------------------------------------------------------------------------------------------------------
// (x, y) the undistorted normalised point (NaN where trk_undistort failed), X the world point.  An unusable correspondence (a NaN
// in x or y, a non-finite X) becomes (NaN, NaN, 0, 0, 0): never an inlier, and a sample that holds it is invalid.
LVBA_TRK_FN void resect_pack(double x, double y, const double *X, double *rec)
{
    const bool ok = x == x && y == y && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
    rec[0] = ok ? x : NAN; rec[1] = ok ? y : NAN;
    rec[2] = ok ? X[0] : 0.0; rec[3] = ok ? X[1] : 0.0; rec[4] = ok ? X[2] : 0.0;
}

// ---- the inlier test ---------------------------------------------------------------------------------------------------------------
LVBA_TRK_FN void resect_transform(const double *R, const double *t, double X0, double X1, double X2, double &cx, double &cy, double &cz)
{
    cx = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    cy = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    cz = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
}
// division-free: the reprojection error in undistorted pixels against rho = max_error_px; false for any NaN
LVBA_TRK_FN bool resect_inlier(const double *R, const double *t, double fx, double fy, double rho, double x, double y, double X0, double X1,
                               double X2)
{
    double cx, cy, cz;
    resect_transform(R, t, X0, X1, X2, cx, cy, cz);
    const double a = fx * (cx - x * cz), b = fy * (cy - y * cz), r = rho * cz;
    return (cz > RESECT_MIN_DEPTH) & (a * a + b * b <= r * r);   // & not &&: no branch in the scoring loop
}

// ---- small fixed-order algebra ----------------------------------------------------------------------------------------------------
// symmetric 3 x 3 as [00 01 02 11 12 22]; its cofactors in the same layout, its determinant along row 0
LVBA_TRK_FN void resect_cof_sym(const double *A, double *C)
{
    C[0] = A[3] * A[5] - A[4] * A[4];
    C[1] = A[4] * A[2] - A[1] * A[5];
    C[2] = A[1] * A[4] - A[3] * A[2];
    C[3] = A[0] * A[5] - A[2] * A[2];
    C[4] = A[1] * A[2] - A[0] * A[4];
    C[5] = A[0] * A[3] - A[1] * A[1];
}
LVBA_TRK_FN double resect_det_sym(const double *A, const double *C) { return (A[0] * C[0] + A[1] * C[1]) + A[2] * C[2]; }
// sum_ij C_ij B_ij of two symmetric matrices
LVBA_TRK_FN double resect_dot_sym(const double *C, const double *B)
{
    return ((C[0] * B[0] + C[3] * B[3]) + C[5] * B[5]) + 2.0 * ((C[1] * B[1] + C[2] * B[2]) + C[4] * B[4]);
}
// u^T A v for symmetric A
LVBA_TRK_FN double resect_form(const double *A, const double *u, const double *v)
{
    const double w0 = (A[0] * v[0] + A[1] * v[1]) + A[2] * v[2];
    const double w1 = (A[1] * v[0] + A[3] * v[1]) + A[4] * v[2];
    const double w2 = (A[2] * v[0] + A[4] * v[1]) + A[5] * v[2];
    return (u[0] * w0 + u[1] * w1) + u[2] * w2;
}
// the inverse of a general 3 x 3 (row-major) by cofactors, the determinant along row 0; no test: a zero determinant gives
// non-finite entries, which the caller's checks catch
LVBA_TRK_FN void resect_inv3(const double *m, double *inv)
{
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    inv[0] = c00 / det; inv[3] = c01 / det; inv[6] = c02 / det;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) / det; inv[4] = (m[0] * m[8] - m[2] * m[6]) / det; inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) / det; inv[5] = (m[2] * m[3] - m[0] * m[5]) / det; inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}
// s_i^2 + s_j^2 - 2 b s_i s_j
LVBA_TRK_FN double resect_side(double si, double sj, double b) { return (si * si + sj * sj) - (2.0 * b) * (si * sj); }

// ---- the minimal solver --------------------------------------------------------------------------------------------------------------
// c0 .. c3: the records of the four draws.  The three depths s_i along the unit bearings f_i = (x_i, y_i, 1) / |.| satisfy
//   s_i^2 + s_j^2 - 2 s_i s_j (f_i . f_j) = a_ij = |X_i - X_j|^2,         s^T M_ij s = a_ij.
// D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 vanish on the solution; so does D0 = D1 + g D2 for every g, and for a root g of
// det(D1 + g D2) = c3 g^3 + c2 g^2 + c1 g + c0 it has rank 2 and is a pair of planes (after Persson and Nordberg, "Lambda twist",
// ECCV 2018; the split below goes through the adjugate instead of their eigenvectors):
//   the root: the cubic made monic (c3 = 0: invalid); with disc = b^2 - 3 c > 0 it has a local maximum at t1 = (-b - sqrt(disc)) / 3
//   and a minimum at t2 = (-b + sqrt(disc)) / 3: where p(t1) > 0 Newton starts left of t1, at t1 - sqrt(p(t1) / sqrt(disc)), else
//   right of t2 at t2 + sqrt(-p(t2) / sqrt(disc)) (the roots of the parabola that osculates p there: from both Newton runs
//   monotonically into the outer root); disc <= 0: from the inflection -b / 3.  RESECT_NEWTON steps, a step with p' = 0 left out.
//   the split: B = -adj(D0) = p p^T with p the planes' common line; i = the largest B_ii (the lowest of a tie; at or below
//   RESECT_SPLIT_REL max|D0|^2: invalid), p = B[:, i] / sqrt(B_ii), N = D0 + [p]x has rank 1; with (r, c) its entry of largest
//   magnitude (row by row, the lowest of a tie) plane 0 is row r of N and plane 1 is column c.
//   per plane n: k = the largest |n_k| (lowest of a tie); two vectors of the plane, (-n1, n0, 0), (-n2, 0, n0) for k = 0,
//   (n1, -n0, 0), (0, -n2, n1) for k = 1, (n2, 0, -n0), (0, n2, -n1) for k = 2; s = al u + be v in D1 is A al^2 + 2 B al be + C be^2
//   = 0; B^2 - A C < 0: no solution of this plane; q = -(B + sign(B) sqrt(.)), root 0 (al, be) = (q, A), root 1 = (C, q): homogeneous,
//   no division.  Solution number 2 plane + root.
//   the scale: lam^2 = (a12 + a13 + a23) / (the three sides of s summed), the sign so that s_1 > 0.
//   RESECT_POLISH Gauss-Newton steps on (s1, s2, s3) against the three equations, the 3 x 3 system by cofactors.
//   a depth that is not finite or not > 0: no solution.
//   R = Y X^-1, X = [X1 - X2, X1 - X3, their cross product], Y the same of s_i f_i, t = s1 f1 - R X1.
// Of the solutions, the one with the smallest squared undistorted-pixel error on the fourth draw, which must lie in front
// (depth > RESECT_MIN_DEPTH); the lowest number of a tie.  false: invalid (R, t zero).
LVBA_TRK_FN bool resect_p3p(const double *c0, const double *c1, const double *c2, const double *c3, double fx, double fy, double *R, double *t)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (!(c0[0] == c0[0] && c1[0] == c1[0] && c2[0] == c2[0] && c3[0] == c3[0])) return false;
    double f[9];
    {
        const double n0 = sqrt((c0[0] * c0[0] + c0[1] * c0[1]) + 1.0), n1 = sqrt((c1[0] * c1[0] + c1[1] * c1[1]) + 1.0),
                     n2 = sqrt((c2[0] * c2[0] + c2[1] * c2[1]) + 1.0);
        f[0] = c0[0] / n0; f[1] = c0[1] / n0; f[2] = 1.0 / n0;
        f[3] = c1[0] / n1; f[4] = c1[1] / n1; f[5] = 1.0 / n1;
        f[6] = c2[0] / n2; f[7] = c2[1] / n2; f[8] = 1.0 / n2;
    }
    const double b12 = (f[0] * f[3] + f[1] * f[4]) + f[2] * f[5], b13 = (f[0] * f[6] + f[1] * f[7]) + f[2] * f[8],
                 b23 = (f[3] * f[6] + f[4] * f[7]) + f[5] * f[8];
    const double d12[3] = {c0[2] - c1[2], c0[3] - c1[3], c0[4] - c1[4]}, d13[3] = {c0[2] - c2[2], c0[3] - c2[3], c0[4] - c2[4]},
                 d23[3] = {c1[2] - c2[2], c1[3] - c2[3], c1[4] - c2[4]};
    const double a12 = (d12[0] * d12[0] + d12[1] * d12[1]) + d12[2] * d12[2], a13 = (d13[0] * d13[0] + d13[1] * d13[1]) + d13[2] * d13[2],
                 a23 = (d23[0] * d23[0] + d23[1] * d23[1]) + d23[2] * d23[2];
    const double cr[3] = {d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0]};
    const double cc = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2];
    if (!(cc > RESECT_TRIANGLE_REL2 * (a12 * a13))) return false;
    const double D1[6] = {a23, -(a23 * b12), 0.0, a23 - a12, a12 * b23, -a12};
    const double D2[6] = {a23, 0.0, -(a23 * b13), -a13, a13 * b23, a23 - a13};
    double g;
    {
        double C1[6], C2[6];
        resect_cof_sym(D1, C1);
        resect_cof_sym(D2, C2);
        const double k0 = resect_det_sym(D1, C1), k1 = resect_dot_sym(C1, D2), k2 = resect_dot_sym(C2, D1), k3 = resect_det_sym(D2, C2);
        if (!(k3 != 0.0)) return false;
        const double b = k2 / k3, c = k1 / k3, d = k0 / k3;
        const double disc = b * b - 3.0 * c;
        if (disc > 0.0) {
            const double v = sqrt(disc);
            const double t1 = (-b - v) / 3.0;
            const double p1 = ((t1 + b) * t1 + c) * t1 + d;
            if (p1 > 0.0) g = t1 - sqrt(p1 / v);
            else {
                const double t2 = (v - b) / 3.0;
                const double p2 = ((t2 + b) * t2 + c) * t2 + d;
                g = t2 + sqrt(-p2 / v);
            }
        } else g = -b / 3.0;
        for (int it = 0; it < RESECT_NEWTON; ++it) {
            const double p = ((g + b) * g + c) * g + d, dp = (3.0 * g + 2.0 * b) * g + c;
            const double step = dp != 0.0 ? p / dp : 0.0;
            g = g - step;
        }
    }
    if (!isfinite(g)) return false;
    double D0[6], n[2][3];
#pragma unroll
    for (int k = 0; k < 6; ++k) D0[k] = D1[k] + g * D2[k];
    {
        double C[6];
        resect_cof_sym(D0, C);
        double scale = fabs(D0[0]);
#pragma unroll
        for (int k = 1; k < 6; ++k) scale = fabs(D0[k]) > scale ? fabs(D0[k]) : scale;
        const double B0 = -C[0], B1 = -C[3], B2 = -C[5];
        int i = 0;
        double bb = B0;
        if (B1 > bb) { bb = B1; i = 1; }
        if (B2 > bb) { bb = B2; i = 2; }
        if (!(bb > RESECT_SPLIT_REL * (scale * scale))) return false;
        const double sb = sqrt(bb);
        const double p0 = -(i == 0 ? C[0] : i == 1 ? C[1] : C[2]) / sb, p1 = -(i == 0 ? C[1] : i == 1 ? C[3] : C[4]) / sb,
                     p2 = -(i == 0 ? C[2] : i == 1 ? C[4] : C[5]) / sb;
        const double N[9] = {D0[0], D0[1] - p2, D0[2] + p1, D0[1] + p2, D0[3], D0[4] - p0, D0[2] - p1, D0[4] + p0, D0[5]};
        double best = -1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = fabs(N[3 * r + c]);
                if (v > best) {
                    best = v;
                    n[0][0] = N[3 * r]; n[0][1] = N[3 * r + 1]; n[0][2] = N[3 * r + 2];
                    n[1][0] = N[c]; n[1][1] = N[3 + c]; n[1][2] = N[6 + c];
                }
            }
        if (!(best > 0.0)) return false;   // also when a NaN is in it
    }
    double Xi[9];
    {
        const double Xm[9] = {d12[0], d13[0], cr[0], d12[1], d13[1], cr[1], d12[2], d13[2], cr[2]};
        resect_inv3(Xm, Xi);
    }
    const double asum = (a12 + a13) + a23;
    double best_err = INFINITY;
    bool found = false;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const double n0 = n[pl][0], n1 = n[pl][1], n2 = n[pl][2];
        int k = 0;
        double nb = fabs(n0);
        if (fabs(n1) > nb) { nb = fabs(n1); k = 1; }
        if (fabs(n2) > nb) { nb = fabs(n2); k = 2; }
        const double u[3] = {k == 0 ? -n1 : k == 1 ? n1 : n2, k == 0 ? n0 : k == 1 ? -n0 : 0.0, k == 2 ? -n0 : 0.0};
        const double v[3] = {k == 0 ? -n2 : 0.0, k == 0 ? 0.0 : k == 1 ? -n2 : n2, k == 0 ? n0 : k == 1 ? n1 : -n1};
        const double qa = resect_form(D1, u, u), qb = resect_form(D1, u, v), qc = resect_form(D1, v, v);
        const double qd = qb * qb - qa * qc;
        if (!(qd >= 0.0)) continue;
        const double sq = sqrt(qd);
        const double q = qb >= 0.0 ? (-qb) - sq : sq - qb;
#pragma unroll
        for (int root = 0; root < 2; ++root) {
            const double al = root == 0 ? q : qc, be = root == 0 ? qa : q;
            double s0 = al * u[0] + be * v[0], s1 = al * u[1] + be * v[1], s2 = al * u[2] + be * v[2];
            const double w = (resect_side(s0, s1, b12) + resect_side(s0, s2, b13)) + resect_side(s1, s2, b23);
            double lam = sqrt(asum / w);
            lam = s0 < 0.0 ? -lam : lam;
            s0 = lam * s0; s1 = lam * s1; s2 = lam * s2;
            for (int it = 0; it < RESECT_POLISH; ++it) {
                const double h0 = 0.5 * (resect_side(s0, s1, b12) - a12), h1 = 0.5 * (resect_side(s0, s2, b13) - a13),
                             h2 = 0.5 * (resect_side(s1, s2, b23) - a23);
                const double J[9] = {s0 - b12 * s1, s1 - b12 * s0, 0.0, s0 - b13 * s2, 0.0, s2 - b13 * s0, 0.0, s1 - b23 * s2, s2 - b23 * s1};
                double Ji[9];
                resect_inv3(J, Ji);
                s0 = s0 - ((Ji[0] * h0 + Ji[1] * h1) + Ji[2] * h2);
                s1 = s1 - ((Ji[3] * h0 + Ji[4] * h1) + Ji[5] * h2);
                s2 = s2 - ((Ji[6] * h0 + Ji[7] * h1) + Ji[8] * h2);
            }
            if (!(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && isfinite(s0) && isfinite(s1) && isfinite(s2))) continue;
            const double y0[3] = {s0 * f[0], s0 * f[1], s0 * f[2]}, y1[3] = {s1 * f[3], s1 * f[4], s1 * f[5]},
                         y2[3] = {s2 * f[6], s2 * f[7], s2 * f[8]};
            const double e1[3] = {y0[0] - y1[0], y0[1] - y1[1], y0[2] - y1[2]}, e2[3] = {y0[0] - y2[0], y0[1] - y2[1], y0[2] - y2[2]};
            const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            double Rs[9], ts[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rs[3 * r + c] = (e1[r] * Xi[c] + e2[r] * Xi[3 + c]) + e3[r] * Xi[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r) ts[r] = y0[r] - ((Rs[3 * r] * c0[2] + Rs[3 * r + 1] * c0[3]) + Rs[3 * r + 2] * c0[4]);
            double px, py, pz;
            resect_transform(Rs, ts, c3[2], c3[3], c3[4], px, py, pz);
            if (!(pz > RESECT_MIN_DEPTH)) continue;
            const double ex = fx * (px / pz - c3[0]), ey = fy * (py / pz - c3[1]);
            const double err = ex * ex + ey * ey;
            if (err < best_err) {
                best_err = err;
                found = true;
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = Rs[e];
                t[0] = ts[0]; t[1] = ts[1]; t[2] = ts[2];
            }
        }
    }
    return found;
}

// ---- the refit -----------------------------------------------------------------------------------------------------------------------
// One correspondence's share of the normal equations at (R, t): r = (fx (Xc_x / Xc_z - x), fy (Xc_y / Xc_z - y)), J its derivative
// by (om, up) of Xc <- Xc + om x Xc + up; acc [RESECT_NSUM] += (J^T J upper triangle by row, J^T r, r . r).  A point at or behind
// the camera under this pose adds nothing.
LVBA_TRK_FN void resect_accumulate(const double *R, const double *t, double fx, double fy, double x, double y, double X0, double X1, double X2,
                                   double *acc)
{
    double cx, cy, cz;
    resect_transform(R, t, X0, X1, X2, cx, cy, cz);
    if (!(cz > RESECT_MIN_DEPTH)) return;
    const double iz = 1.0 / cz, px = cx * iz, py = cy * iz;
    const double r0 = fx * (px - x), r1 = fy * (py - y);
    const double gx = fx * iz, gy = fy * iz, gz0 = -(gx * px), gz1 = -(gy * py);
    const double J0[6] = {gz0 * cy, gx * cz - gz0 * cx, -(gx * cy), gx, 0.0, gz0};
    const double J1[6] = {gz1 * cy - gy * cz, -(gz1 * cx), gy * cx, 0.0, gy, gz1};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) acc[k++] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] += J0[r] * r0 + J1[r] * r1;
    acc[27] += r0 * r0 + r1 * r1;
}
// N d = g for the symmetric positive definite 6 x 6 N (full storage; destroyed) by Cholesky, column after column; false: a pivot that
// is not > 0 or not finite.  Every loop has a constant trip count: the device build unrolls them and keeps N in registers.
LVBA_TRK_FN bool resect_solve6(double *N, const double *g, double *d)
{
    for (int j = 0; j < 6; ++j) {
        double p = N[7 * j];
        for (int k = 0; k < j; ++k) p -= N[6 * j + k] * N[6 * j + k];
        if (!(p > 0.0) || !isfinite(p)) return false;
        p = sqrt(p);
        N[7 * j] = p;
        for (int i = j + 1; i < 6; ++i) {
            double v = N[6 * i + j];
            for (int k = 0; k < j; ++k) v -= N[6 * i + k] * N[6 * j + k];
            N[6 * i + j] = v / p;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = g[i];
        for (int k = 0; k < i; ++k) v -= N[6 * i + k] * y[k];
        y[i] = v / N[7 * i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= N[6 * k + i] * d[k];
        d[i] = v / N[7 * i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(d[i])) return false;
    return true;
}
// R to the nearest-by rotation through a unit quaternion (the largest of trace, R00, R11, R22 picks the branch; sqrt only)
LVBA_TRK_FN void resect_orthonormalise(double *R)
{
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) { w = 1.0 + tr; x = R[7] - R[5]; y = R[2] - R[6]; z = R[3] - R[1]; }
    else if (R[0] >= R[4] && R[0] >= R[8]) { w = R[7] - R[5]; x = 1.0 + R[0] - R[4] - R[8]; y = R[1] + R[3]; z = R[2] + R[6]; }
    else if (R[4] >= R[8]) { w = R[2] - R[6]; x = R[1] + R[3]; y = 1.0 - R[0] + R[4] - R[8]; z = R[5] + R[7]; }
    else { w = R[3] - R[1]; x = R[2] + R[6]; y = R[5] + R[7]; z = 1.0 - R[0] - R[4] + R[8]; }
    const double n = sqrt(w * w + x * x + y * y + z * z);
    if (!(n > 0.0) || !isfinite(n)) return;
    w /= n; x /= n; y /= n; z /= n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
// One Gauss-Newton step from the sums: d = -(J^T J)^-1 J^T r, R <- (I + [om]x) R re-orthonormalised, t <- t + om x t + up.
// N36 [36] is workspace (see resect_solve6).  false: no step, (R, t) untouched.
LVBA_TRK_FN bool resect_step(const double *acc, double *N36, double *R, double *t)
{
    int k = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) { N36[6 * r + c] = acc[k]; N36[6 * c + r] = acc[k]; ++k; }
    double g[6], d[6];
    for (int r = 0; r < 6; ++r) g[r] = -acc[21 + r];
    if (!resect_solve6(N36, g, d)) return false;
    double Rn[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Rn[c] = R[c] + (d[1] * R[6 + c] - d[2] * R[3 + c]);
        Rn[3 + c] = R[3 + c] + (d[2] * R[c] - d[0] * R[6 + c]);
        Rn[6 + c] = R[6 + c] + (d[0] * R[3 + c] - d[1] * R[c]);
    }
    const double tn[3] = {t[0] + (d[1] * t[2] - d[2] * t[1]) + d[3], t[1] + (d[2] * t[0] - d[0] * t[2]) + d[4],
                          t[2] + (d[0] * t[1] - d[1] * t[0]) + d[5]};
    resect_orthonormalise(Rn);
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rn[e];
    t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
    return true;
}

} // namespace lvba
