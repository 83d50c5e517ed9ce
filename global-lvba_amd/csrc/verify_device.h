// verify_device.h -- the two-view pieces of the verification of putative matches (verify.hip; the rule is in include/lvba_hip.h,
// DESIGN.md §10k): the inlier tests, the minimal solvers (eight points, two points with the rotation, four points for the
// homography) and the refits over the inliers (cyclic Jacobi, projection onto the essential manifold).  The generator, the
// sampler, the rank and the status are ransac_device.h'.  Host/device-neutral, like match_device.h, whose gate it uses as it stands: a match is an inlier of E exactly where the guided matcher would pass it.
// The solvers use +, -, *, / and sqrt only, in the order written here, and verify.hip is built without contraction: a hypothesis
// is the same bits on the host and on the device.  The refits go through eig3 and long rotation chains and are held to a
// measured tolerance instead.
#pragma once
#include <math.h>
#include <stdint.h>
#include "match_device.h"
#include "balm_math.h"
#include "ransac_device.h"

namespace lvba {

enum VerifyMethod : int { VERIFY_EIGHT_POINT = 0, VERIFY_KNOWN_ROTATION = 1 };                       // lvba_verify_opts::method
// The homography is no lvba_verify_opts::method (lvba_verify_pairs refuses 2): it is what the kernels of verify.hip are
// instantiated with for LVBA_VERIFY_MODEL_HOMOGRAPHY.
constexpr int VERIFY_HOMOGRAPHY = 2;
enum VerifyModel : int { VERIFY_MODEL_ESSENTIAL = 0, VERIFY_MODEL_HOMOGRAPHY = 1, VERIFY_MODEL_AUTO = 2 };   // lvba_verify_pairs_model
constexpr double VERIFY_PLANAR_RATIO = 0.8;       // the default of planar_ratio: COLMAP's max_H_inlier_ratio
constexpr int VERIFY_OK = RANSAC_OK, VERIFY_TOO_FEW_MATCHES = RANSAC_TOO_FEW_MATCHES, VERIFY_NO_MODEL = RANSAC_NO_MODEL,
              VERIFY_TOO_FEW_INLIERS = RANSAC_TOO_FEW_INLIERS;
// A pivot at or below this share of the system's largest entry is "no pivot".  The rounding of an eight-step elimination of
// entries of order 1 is ~1e-15 and a usable sample's last pivot is above ~1e-6: five decades of room on either side.
constexpr double VERIFY_PIVOT_REL = 1e-10;
// |c1 x c2|^2 <= this |c1|^2 |c2|^2 (sin^2 of the angle between the two constraints): no direction.  As MATCH_BASELINE_REL2.
constexpr double VERIFY_T_REL2 = 1e-20;
constexpr int VERIFY_JACOBI_SWEEPS = 12;          // cyclic Jacobi on the 9 x 9 normal matrix: converged after 7 or 8 on every fixture

LVBA_TRK_FN int verify_sample_size(int method) { return method == VERIFY_KNOWN_ROTATION ? 2 : method == VERIFY_HOMOGRAPHY ? 4 : 8; }
// The E-or-H choice of one pair from its two finished runs: HOMOGRAPHY iff the H run is OK and either the E run is not, or
// n_H >= planar_ratio n_E in fp64.
LVBA_TRK_FN int verify_choose_model(int status_E, int32_t n_E, int status_H, int32_t n_H, double planar_ratio)
{
    return status_H == RANSAC_OK && (status_E != RANSAC_OK || (double)n_H >= planar_ratio * (double)n_E) ? VERIFY_MODEL_HOMOGRAPHY
                                                                                                           : VERIFY_MODEL_ESSENTIAL;
}

// ---- the inlier test: the guided matcher's gate -------------------------------------------------------------------------------
// p = (x_lo, y_lo, x_hi, y_hi); false when a NaN (failed undistortion) is in it
LVBA_TRK_FN bool verify_inlier(const double *E, double xl, double yl, double xh, double yh, double tau2)
{
    return match_gate(match_line_lo(E, xl, yl), xh, yh, match_norm_hi(E, xh, yh), tau2);
}
// E scaled to unit Frobenius norm, the squares summed left to right; false (E untouched) when the norm is 0 or not finite
LVBA_TRK_FN bool verify_unit(double *E)
{
    double n2 = E[0] * E[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) n2 = n2 + E[k] * E[k];
    const double n = sqrt(n2);
    if (!(n > 0.0) || !isfinite(n)) return false;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = E[k] / n;
    return true;
}
LVBA_TRK_FN void verify_zero(double *E)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
}

// ---- method 0: eight points, no pose ------------------------------------------------------------------------------------------
// The 8 x 9 system lives at A[(9 r + c) st]: st = 1 on the host, the workgroup's width on the device, where lane l starts at
// A + l and its 72 entries sit in LDS without a bank conflict.  Row r is x^_hi (x) x^_lo, so that a . vec(E) = x^_hi^T E x^_lo.
// Returns false when the point holds a NaN.
LVBA_TRK_FN bool verify_eight_row(double *A, int st, int r, double xl, double yl, double xh, double yh)
{
    double *a = A + 9 * r * st;
    a[0] = xh * xl; a[st] = xh * yl; a[2 * st] = xh;
    a[3 * st] = yh * xl; a[4 * st] = yh * yl; a[5 * st] = yh;
    a[6 * st] = xl; a[7 * st] = yl; a[8 * st] = 1.0;
    return xl == xl && yl == yl && xh == xh && yh == yh;
}
// The null vector of the 8 x 9 system by Gauss-Jordan elimination with full pivoting, in this order of operations:
//   scale = the largest |entry|;  for s = 0 .. 7:  the pivot is the largest |A[r][c]| over r in s .. 7, c in s .. 8, scanned row
//   by row, a strict > so that the lowest (r, c) wins a tie;  no pivot (<= VERIFY_PIVOT_REL scale, or a NaN): invalid;  rows s
//   and r are exchanged, then columns s and c (and the column's name);  A[s][c] /= pivot for c > s;  A[r][c] -= A[r][s] A[s][c]
//   for every other row r and c > s.
// Then vec(E) is 1 at the column left over, -A[i][8] at the column that pivot i eliminated, and is scaled to unit norm.
// Degenerate where the scene is one plane (the system has rank 6 there and no pivot test can tell which null vector is the
// geometry): that is what the rotation-aided method is for.  A is destroyed.  false: invalid, E = 0.
LVBA_TRK_FN bool verify_eight_solve(double *A, int st, double *E)
{
#define LVBA_VA(r, c) A[(9 * (r) + (c)) * st]
    double scale = 0.0;
    for (int e = 0; e < 72; ++e) {
        const double v = fabs(A[e * st]);
        scale = v > scale ? v : scale;
    }
    uint64_t perm = 0x876543210ull;                // nibble c: the unknown that column c stands for
    for (int s = 0; s < 8; ++s) {
        double best = -1.0;
        int pr = s, pc = s;
        for (int r = s; r < 8; ++r)
            for (int c = s; c < 9; ++c) {
                const double v = fabs(LVBA_VA(r, c));
                if (v > best) { best = v; pr = r; pc = c; }
            }
        if (!(best > VERIFY_PIVOT_REL * scale)) { verify_zero(E); return false; }
        if (pr != s)
            for (int c = 0; c < 9; ++c) { const double x = LVBA_VA(s, c); LVBA_VA(s, c) = LVBA_VA(pr, c); LVBA_VA(pr, c) = x; }
        if (pc != s) {
            for (int r = 0; r < 8; ++r) { const double x = LVBA_VA(r, s); LVBA_VA(r, s) = LVBA_VA(r, pc); LVBA_VA(r, pc) = x; }
            const uint64_t ns = (perm >> (4 * s)) & 15, nc = (perm >> (4 * pc)) & 15;
            perm = (perm & ~((15ull << (4 * s)) | (15ull << (4 * pc)))) | (nc << (4 * s)) | (ns << (4 * pc));
        }
        const double p = LVBA_VA(s, s);
        for (int c = s + 1; c < 9; ++c) LVBA_VA(s, c) = LVBA_VA(s, c) / p;
        for (int r = 0; r < 8; ++r) {
            if (r == s) continue;
            const double f = LVBA_VA(r, s);
            for (int c = s + 1; c < 9; ++c) LVBA_VA(r, c) = LVBA_VA(r, c) - f * LVBA_VA(s, c);
        }
    }
    double v[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = -LVBA_VA(i, 8);
    v[8] = 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) A[(int)((perm >> (4 * i)) & 15) * st] = v[i];   // row 0 is free now: vec(E) by unknown
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = A[k * st];
#undef LVBA_VA
    if (!verify_unit(E)) { verify_zero(E); return false; }
    return true;
}

// ---- method 1: two points, the relative rotation known ------------------------------------------------------------------------
// R = R_hi R_lo^T, every sum left to right (match_essential's expression)
LVBA_TRK_FN void verify_relative_rotation(const double *Rlo, const double *Rhi, double *R)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Rhi[3 * i] * Rlo[3 * j] + Rhi[3 * i + 1] * Rlo[3 * j + 1]) + Rhi[3 * i + 2] * Rlo[3 * j + 2];
}
// c = x^_hi x (R x^_lo): the translation direction is orthogonal to it
LVBA_TRK_FN void verify_constraint(const double *R, double xl, double yl, double xh, double yh, double *c)
{
    const double q0 = (R[0] * xl + R[1] * yl) + R[2], q1 = (R[3] * xl + R[4] * yl) + R[5], q2 = (R[6] * xl + R[7] * yl) + R[8];
    c[0] = yh * q2 - q1;
    c[1] = q0 - xh * q2;
    c[2] = xh * q1 - yh * q0;
}
// E = [t]x R, unit norm
LVBA_TRK_FN bool verify_essential_from(const double *t, const double *R, double *E)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
    if (!verify_unit(E)) { verify_zero(E); return false; }
    return true;
}
// p = the two sample points, (x_lo, y_lo, x_hi, y_hi) each.  false: invalid (a NaN, or the two constraints parallel), E = 0.
LVBA_TRK_FN bool verify_known_rotation(const double *p, const double *R, double *E)
{
    double c1[3], c2[3], t[3];
    verify_constraint(R, p[0], p[1], p[2], p[3], c1);
    verify_constraint(R, p[4], p[5], p[6], p[7], c2);
    t[0] = c1[1] * c2[2] - c1[2] * c2[1];
    t[1] = c1[2] * c2[0] - c1[0] * c2[2];
    t[2] = c1[0] * c2[1] - c1[1] * c2[0];
    const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    const double n1 = (c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2], n2 = (c2[0] * c2[0] + c2[1] * c2[1]) + c2[2] * c2[2];
    if (!(tt > VERIFY_T_REL2 * (n1 * n2))) { verify_zero(E); return false; }   // also when a NaN is in it
    return verify_essential_from(t, R, E);
}

// ---- the homography: four points, no pose, for a scene that is one plane ------------------------------------------------------
// H maps lo to hi, p = H x^_lo ~ x^_hi.  Sample point i fills rows 2 i and 2 i + 1 of the 8 x 9 system of verify_eight_solve
// (same layout, same st): p0 - x_hi p2 = 0 and p1 - y_hi p2 = 0.  Returns false when the point holds a NaN.
LVBA_TRK_FN bool verify_homography_rows(double *A, int st, int i, double xl, double yl, double xh, double yh)
{
    double *a = A + 18 * i * st, *b = a + 9 * st;
    a[0] = xl; a[st] = yl; a[2 * st] = 1.0; a[3 * st] = 0.0; a[4 * st] = 0.0; a[5 * st] = 0.0;
    a[6 * st] = -xh * xl; a[7 * st] = -xh * yl; a[8 * st] = -xh;
    b[0] = 0.0; b[st] = 0.0; b[2 * st] = 0.0; b[3 * st] = xl; b[4 * st] = yl; b[5 * st] = 1.0;
    b[6 * st] = -yh * xl; b[7 * st] = -yh * yl; b[8 * st] = -yh;
    return xl == xl && yl == yl && xh == xh && yh == yh;
}
// The sign of H: negated if the third coordinate of H x^_lo is negative at (xl, yl), the first sample point.  false (H = 0)
// when it is zero or a NaN there.
LVBA_TRK_FN bool verify_homography_sign(double *H, double xl, double yl)
{
    const double p2 = (H[6] * xl + H[7] * yl) + H[8];
    if (!(p2 > 0.0) && !(p2 < 0.0)) { verify_zero(H); return false; }
    if (p2 < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = -H[k];
    }
    return true;
}
// G = adj(H), negated if det H < 0: a positive multiple of H^-1.  det H = (H0 G0 + H1 G3) + H2 G6, the first row of H on the
// first column of adj(H).  false (G = 0) when det H is zero or not finite.
LVBA_TRK_FN bool verify_homography_inverse(const double *H, double *G)
{
    G[0] = H[4] * H[8] - H[5] * H[7]; G[1] = H[2] * H[7] - H[1] * H[8]; G[2] = H[1] * H[5] - H[2] * H[4];
    G[3] = H[5] * H[6] - H[3] * H[8]; G[4] = H[0] * H[8] - H[2] * H[6]; G[5] = H[2] * H[3] - H[0] * H[5];
    G[6] = H[3] * H[7] - H[4] * H[6]; G[7] = H[1] * H[6] - H[0] * H[7]; G[8] = H[0] * H[4] - H[1] * H[3];
    const double det = (H[0] * G[0] + H[1] * G[3]) + H[2] * G[6];
    if (!isfinite(det) || det == 0.0) { verify_zero(G); return false; }
    if (det < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k] = -G[k];
    }
    return true;
}
// one direction of the transfer test: x^ = (x, y, 1) carried by M lands within tau of (u, v), in front of the camera
LVBA_TRK_FN bool verify_transfer(const double *M, double x, double y, double u, double v, double tau2)
{
    const double p0 = (M[0] * x + M[1] * y) + M[2], p1 = (M[3] * x + M[4] * y) + M[5], p2 = (M[6] * x + M[7] * y) + M[8];
    const double d0 = p0 - u * p2, d1 = p1 - v * p2;
    const bool near = d0 * d0 + d1 * d1 <= tau2 * (p2 * p2), front = p2 > 0.0;
    return near & front;            // no branch: the scoring loop stays one block
}
// the symmetric transfer test: lo carried to hi by H and hi carried to lo by G, both within tau; false when a NaN is in it
LVBA_TRK_FN bool verify_inlier_h(const double *H, const double *G, double xl, double yl, double xh, double yh, double tau2)
{
    const bool there = verify_transfer(H, xl, yl, xh, yh, tau2), back = verify_transfer(G, xh, yh, xl, yl, tau2);
    return there & back;
}
// H and G of the four sample points whose rows are in A (verify_homography_rows); (xl, yl) is the first of them.
// false: invalid, H = G = 0.
LVBA_TRK_FN bool verify_homography_solve(double *A, int st, double xl, double yl, double *H, double *G)
{
    verify_zero(G);
    if (!verify_eight_solve(A, st, H)) return false;
    if (!verify_homography_sign(H, xl, yl)) return false;
    if (!verify_homography_inverse(H, G)) { verify_zero(H); return false; }
    return true;
}

// ---- local refinement --------------------------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric n x n matrix A (full storage, row-major; plain memory, LDS on the device, so that p and q may
// be run-time indices): VERIFY_JACOBI_SWEEPS sweeps over (p, q), p < q, in row order, tracks_device.h' rotation with IEEE
// divisions and square roots; V = the eigenvectors by column, A's diagonal the eigenvalues.
LVBA_TRK_FN void verify_jacobi(double *A, double *V, int n)
{
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) V[n * r + c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < VERIFY_JACOBI_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off += fabs(A[n * p + q]);
        if (off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[n * p + q];
                if (apq == 0.0) continue;
                const double th = (A[n * q + q] - A[n * p + p]) / (2.0 * apq);
                const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int r = 0; r < n; ++r) {
                    const double arp = A[n * r + p], arq = A[n * r + q];
                    A[n * r + p] = cs * arp - sn * arq;
                    A[n * r + q] = sn * arp + cs * arq;
                }
                for (int r = 0; r < n; ++r) {
                    const double apr = A[n * p + r], aqr = A[n * q + r];
                    A[n * p + r] = cs * apr - sn * aqr;
                    A[n * q + r] = sn * apr + cs * aqr;
                }
                A[n * p + q] = 0.0; A[n * q + p] = 0.0;
                for (int r = 0; r < n; ++r) {
                    const double vrp = V[n * r + p], vrq = V[n * r + q];
                    V[n * r + p] = cs * vrp - sn * vrq;
                    V[n * r + q] = sn * vrp + cs * vrq;
                }
            }
    }
}
// E onto the essential manifold (two equal singular values, one zero), up to scale: with E^T E = sum lam_i v_i v_i^T (eig3,
// ascending) the nearest such matrix is a multiple of E (v_1 v_1^T / s_1 + v_2 v_2^T / s_2), s_i = sqrt(lam_i); then unit norm.
LVBA_TRK_FN bool verify_project(double *E)
{
    double C[6], lam[3], U[9];
    int k = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) C[k++] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    eig3<true, false>(C, lam, U);
    if (!(lam[1] > 0.0) || !isfinite(lam[2])) return false;
    const double s1 = sqrt(lam[1]), s2 = sqrt(lam[2]);
    double P[9], F[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P[3 * i + j] = U[3 * i + 1] * U[3 * j + 1] / s1 + U[3 * i + 2] * U[3 * j + 2] / s2;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = (E[3 * i] * P[j] + E[3 * i + 1] * P[3 + j]) + E[3 * i + 2] * P[6 + j];
    if (!verify_unit(F)) return false;
    for (int e = 0; e < 9; ++e) E[e] = F[e];
    return true;
}
// The refit of method 0: N = sum a a^T over the inliers (9 x 9, full storage; destroyed), V [81] workspace.  E = the eigenvector
// of N's smallest eigenvalue (the lowest column of a tie), projected.  false: no refit, E untouched.
LVBA_TRK_FN bool verify_refit_eight(double *N, double *V, double *E)
{
    verify_jacobi(N, V, 9);
    int mn = 0;
    for (int c = 1; c < 9; ++c)
        if (N[10 * c] < N[10 * mn]) mn = c;
    double F[9];
    for (int r = 0; r < 9; ++r) F[r] = V[9 * r + mn];
    for (int r = 0; r < 9; ++r)
        if (!isfinite(F[r])) return false;
    if (!verify_project(F)) return false;
    for (int r = 0; r < 9; ++r) E[r] = F[r];
    return true;
}
// The refit of method 1: C = sum c c^T over the inliers as [c00 c01 c02 c11 c12 c22]; t = its smallest eigenvector.
LVBA_TRK_FN bool verify_refit_rotation(const double *C, const double *R, double *E)
{
    double lam[3], U[9], F[9];
    for (int k = 0; k < 6; ++k)
        if (!isfinite(C[k])) return false;
    eig3<true, false>(C, lam, U);
    const double t[3] = {U[0], U[3], U[6]};
    if (!verify_essential_from(t, R, F)) return false;
    for (int r = 0; r < 9; ++r) E[r] = F[r];
    return true;
}
// The two rows of one match in the homography's system, as verify_homography_rows writes them.
LVBA_TRK_FN void verify_homography_row_pair(double xl, double yl, double xh, double yh, double *r1, double *r2)
{
    r1[0] = xl; r1[1] = yl; r1[2] = 1.0; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0; r1[6] = -xh * xl; r1[7] = -xh * yl; r1[8] = -xh;
    r2[0] = 0.0; r2[1] = 0.0; r2[2] = 0.0; r2[3] = xl; r2[4] = yl; r2[5] = 1.0; r2[6] = -yh * xl; r2[7] = -yh * yl; r2[8] = -yh;
}
// The refit of the homography: N = sum (r1 r1^T + r2 r2^T) over the inliers (9 x 9, full storage; destroyed), V [81] workspace.
// H = the eigenvector of N's smallest eigenvalue (the lowest column of a tie), unit norm, negated if its inner product with the
// current H is negative; not projected.  G = its inverse direction.  false: no refit, H and G untouched.
LVBA_TRK_FN bool verify_refit_homography(double *N, double *V, double *H, double *G)
{
    verify_jacobi(N, V, 9);
    int mn = 0;
    for (int c = 1; c < 9; ++c)
        if (N[10 * c] < N[10 * mn]) mn = c;
    double F[9], Gn[9];
    for (int r = 0; r < 9; ++r) F[r] = V[9 * r + mn];
    for (int r = 0; r < 9; ++r)
        if (!isfinite(F[r])) return false;
    if (!verify_unit(F)) return false;
    double dot = F[0] * H[0];
    for (int r = 1; r < 9; ++r) dot = dot + F[r] * H[r];
    if (dot < 0.0)
        for (int r = 0; r < 9; ++r) F[r] = -F[r];
    if (!verify_homography_inverse(F, Gn)) return false;
    for (int r = 0; r < 9; ++r) { H[r] = F[r]; G[r] = Gn[r]; }
    return true;
}

} // namespace lvba
