// prior_device.h -- pose priors of the LiDAR bundle adjustment (lvba_balm_set_priors).  Also compiles as plain C++
// (tests/prior_check.cpp).
//   A pose is T = (R, p); the update is BALM's retraction R <- R Exp(dphi), p <- p + dp (bavoxel.hpp:723-727), d = [phi; p].
//   A prior k has a 6 x 6 square-root information L (row-major) and body-frame offsets O = (R_O, p_O); A = T_i O_i, B = T_j O_j:
//     POSE      r = [Log(Rm^T R_A); p_A - pm]                              (6 rows)
//     POSITION  r = p_A - z                                                (3 rows, top-left 3 x 3 of L)
//     RELATIVE  r = [Log(Rm^T R_A^T R_B); R_A^T (p_B - p_A) - pm]          (6 rows)
//   and adds 1/2 |L r|^2 to the cost.  prior_raw gives r and the Jacobian blocks dr/dd_i, dr/dd_j (row-major 6 x 6; POSITION:
//   rows 3..5 zero); prior_whiten / prior_whiten_jac apply L.
//   One edge is prior_eval (e, 1/2 |e|^2, the whitened blocks) and then prior_record (the lin record PL_*): the LiDAR priors
//   (priors.hip) and the pose graph's edges (posegraph_device.h: its loss scales in between).  The visual stage's priors
//   (visual_prior_device.h, visual_priors.hip) share the model above, prior_record and, device only, prior_grid_sum.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LVBA_HD __host__ __device__ __forceinline__
#define LVBA_PRIOR_UNROLL _Pragma("unroll")
#else
#define LVBA_PRIOR_UNROLL
#ifndef LVBA_HD
#define LVBA_HD inline
#endif
#endif

namespace lvba {

// kinds: the LVBA_PRIOR_* values of include/lvba_hip.h
enum { PRIOR_POSE = 0, PRIOR_POSITION = 1, PRIOR_RELATIVE = 2 };

// C = A B, C = A^T B, C = A B^T (3 x 3 row-major)
LVBA_HD void m3_mul(const double *A, const double *B, double *C)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
LVBA_HD void m3_tmul(const double *A, const double *B, double *C)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
LVBA_HD void m3_mult(const double *A, const double *B, double *C)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
LVBA_HD void m3_vec(const double *A, const double *v, double *o)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
LVBA_HD void m3_tvec(const double *A, const double *v, double *o)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r) o[r] = A[r] * v[0] + A[3 + r] * v[1] + A[6 + r] * v[2];
}
// C = A [v]x
LVBA_HD void m3_mul_hat(const double *A, const double *v, double *C)
{
LVBA_PRIOR_UNROLL
    for (int r = 0; r < 3; ++r) {
        const double a0 = A[3 * r], a1 = A[3 * r + 1], a2 = A[3 * r + 2];
        C[3 * r] = a1 * v[2] - a2 * v[1];
        C[3 * r + 1] = a2 * v[0] - a0 * v[2];
        C[3 * r + 2] = a0 * v[1] - a1 * v[0];
    }
}

// Log of SO(3), accurate near 0 and near pi: theta = atan2(|w|, (tr - 1) / 2), w = vee(R - R^T) / 2; near pi the axis comes
// from the symmetric part (R + R^T) / 2 - cos(theta) I = (1 - cos(theta)) a a^T, signed by w.
LVBA_HD void so3_log(const double *R, double *phi)
{
    const double w0 = 0.5 * (R[7] - R[5]), w1 = 0.5 * (R[2] - R[6]), w2 = 0.5 * (R[3] - R[1]);
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double s = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double th = atan2(s, c);
    if (c > -0.9) {
        double f; // theta / sin(theta)
        if (th < 1e-4) { const double t2 = th * th; f = 1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0; }
        else f = th / s;
        phi[0] = f * w0; phi[1] = f * w1; phi[2] = f * w2;
        return;
    }
    const double S00 = R[0] - c, S11 = R[4] - c, S22 = R[8] - c;
    int k = 0;
    if (S11 > S00 && S11 >= S22) k = 1;
    else if (S22 > S00 && S22 > S11) k = 2;
    double a0, a1, a2;
    if (k == 0) { a0 = S00; a1 = 0.5 * (R[1] + R[3]); a2 = 0.5 * (R[2] + R[6]); }
    else if (k == 1) { a0 = 0.5 * (R[1] + R[3]); a1 = S11; a2 = 0.5 * (R[5] + R[7]); }
    else { a0 = 0.5 * (R[2] + R[6]); a1 = 0.5 * (R[5] + R[7]); a2 = S22; }
    double n = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    if (a0 * w0 + a1 * w1 + a2 * w2 < 0.0) n = -n;
    const double f = th / n;
    phi[0] = f * a0; phi[1] = f * a1; phi[2] = f * a2;
}

// Rodrigues
LVBA_HD void so3_exp(const double *w, double *R)
{
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(t2);
    double A, B; // sin(th) / th, (1 - cos(th)) / th^2
    if (th < 1e-4) { A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0; B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0; }
    else { A = sin(th) / th; const double h = sin(0.5 * th) / th; B = 2.0 * h * h; }
    R[0] = 1.0 - B * (w[1] * w[1] + w[2] * w[2]);
    R[4] = 1.0 - B * (w[0] * w[0] + w[2] * w[2]);
    R[8] = 1.0 - B * (w[0] * w[0] + w[1] * w[1]);
    R[1] = -A * w[2] + B * w[0] * w[1]; R[3] = A * w[2] + B * w[0] * w[1];
    R[2] = A * w[1] + B * w[0] * w[2];  R[6] = -A * w[1] + B * w[0] * w[2];
    R[5] = -A * w[0] + B * w[1] * w[2]; R[7] = A * w[0] + B * w[1] * w[2];
}

// Jr^-1(phi) = I + 1/2 [phi]x + (1/th^2 - cot(th/2) / (2 th)) [phi]x^2  (finite at th = pi)
LVBA_HD void so3_jr_inv(const double *p, double *J)
{
    const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const double th = sqrt(t2);
    double b;
    if (th < 1e-2) b = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
    else b = 1.0 / t2 - cos(0.5 * th) / (2.0 * th * sin(0.5 * th));
    // [p]x^2 = p p^T - t2 I
    J[0] = 1.0 + b * (p[0] * p[0] - t2); J[4] = 1.0 + b * (p[1] * p[1] - t2); J[8] = 1.0 + b * (p[2] * p[2] - t2);
    J[1] = -0.5 * p[2] + b * p[0] * p[1]; J[3] = 0.5 * p[2] + b * p[0] * p[1];
    J[2] = 0.5 * p[1] + b * p[0] * p[2];  J[6] = -0.5 * p[1] + b * p[0] * p[2];
    J[5] = -0.5 * p[0] + b * p[1] * p[2]; J[7] = 0.5 * p[0] + b * p[1] * p[2];
}

// A = T O (poses as R row-major | t)
LVBA_HD void prior_compose(const double *T, const double *O, double *RA, double *pA)
{
    m3_mul(T, O, RA);
    m3_vec(T, O + 9, pA);
    pA[0] += T[9]; pA[1] += T[10]; pA[2] += T[11];
}

// The raw residual r (6; POSITION: r[0..2] = p_A - z, r[3..5] = 0) and, when jac, the raw Jacobian blocks dr/dd_i, dr/dd_j
// (row-major 6 x 6; Jj: RELATIVE only).  Ti / Tj: the poses (Tj unused unless RELATIVE).  (A flag, not a test of Ji against NULL:
// comparing a local array's address keeps it out of registers on the device.)
LVBA_HD void prior_raw(int kind, const double *meas, const double *Ti, const double *Oi, const double *Tj, const double *Oj, double *r,
                       bool jac, double *Ji, double *Jj)
{
    double RA[9], pA[3];
    prior_compose(Ti, Oi, RA, pA);
    if (kind == PRIOR_POSITION) {
        r[0] = pA[0] - meas[9]; r[1] = pA[1] - meas[10]; r[2] = pA[2] - meas[11];
        r[3] = r[4] = r[5] = 0.0;
        if (jac) {
            double M[9];
            m3_mul_hat(Ti, Oi + 9, M); // R_i [p_O]x
LVBA_PRIOR_UNROLL
            for (int a = 0; a < 36; ++a) Ji[a] = 0.0;
LVBA_PRIOR_UNROLL
            for (int rr = 0; rr < 3; ++rr) {
LVBA_PRIOR_UNROLL
                for (int c = 0; c < 3; ++c) Ji[6 * rr + c] = -M[3 * rr + c];
                Ji[6 * rr + 3 + rr] = 1.0;
            }
        }
        return;
    }
    if (kind == PRIOR_POSE) {
        double E[9];
        m3_tmul(meas, RA, E); // Rm^T R_A
        so3_log(E, r);
        r[3] = pA[0] - meas[9]; r[4] = pA[1] - meas[10]; r[5] = pA[2] - meas[11];
        if (jac) {
            double Jr[9], M[9], N[9];
            so3_jr_inv(r, Jr);
            m3_mult(Jr, Oi, M);        // Jr^-1 R_O^T
            m3_mul_hat(Ti, Oi + 9, N); // R_i [p_O]x
LVBA_PRIOR_UNROLL
            for (int rr = 0; rr < 3; ++rr)
LVBA_PRIOR_UNROLL
                for (int c = 0; c < 3; ++c) {
                    Ji[6 * rr + c] = M[3 * rr + c];
                    Ji[6 * rr + 3 + c] = 0.0;
                    Ji[6 * (rr + 3) + c] = -N[3 * rr + c];
                    Ji[6 * (rr + 3) + 3 + c] = rr == c ? 1.0 : 0.0;
                }
        }
        return;
    }
    // RELATIVE
    double RB[9], pB[3], Mr[9], E[9], d[3], q[3];
    prior_compose(Tj, Oj, RB, pB);
    m3_tmul(RA, RB, Mr);  // R_A^T R_B
    m3_tmul(meas, Mr, E); // Rm^T R_A^T R_B
    so3_log(E, r);
    d[0] = pB[0] - pA[0]; d[1] = pB[1] - pA[1]; d[2] = pB[2] - pA[2];
    m3_tvec(RA, d, q); // R_A^T d
    r[3] = q[0] - meas[9]; r[4] = q[1] - meas[10]; r[5] = q[2] - meas[11];
    if (!jac) return;
    double Jr[9], T1[9], T2[9], T3[9];
    so3_jr_inv(r, Jr);
    // pose i: rotation -Jr^-1 Mr^T R_Oi^T;  position [q]x R_Oi^T + R_Oi^T [p_Oi]x, dp: -R_A^T
    {
        double MtRo[9]; // Mr^T R_Oi^T = (R_Oi Mr)^T
        m3_mul(Oi, Mr, T2);
LVBA_PRIOR_UNROLL
        for (int a = 0; a < 3; ++a)
LVBA_PRIOR_UNROLL
            for (int b = 0; b < 3; ++b) MtRo[3 * a + b] = T2[3 * b + a];
        m3_mul(Jr, MtRo, T1); // Jr^-1 Mr^T R_Oi^T
    }
    {
        const double qh[9] = {0.0, -q[2], q[1], q[2], 0.0, -q[0], -q[1], q[0], 0.0};
        m3_mult(qh, Oi, T2); // [q]x R_Oi^T
        double RoT[9];
LVBA_PRIOR_UNROLL
        for (int a = 0; a < 3; ++a)
LVBA_PRIOR_UNROLL
            for (int b = 0; b < 3; ++b) RoT[3 * a + b] = Oi[3 * b + a];
        m3_mul_hat(RoT, Oi + 9, T3); // R_Oi^T [p_Oi]x
    }
LVBA_PRIOR_UNROLL
    for (int rr = 0; rr < 3; ++rr)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) {
            Ji[6 * rr + c] = -T1[3 * rr + c];
            Ji[6 * rr + 3 + c] = 0.0;
            Ji[6 * (rr + 3) + c] = T2[3 * rr + c] + T3[3 * rr + c];
            Ji[6 * (rr + 3) + 3 + c] = -RA[3 * c + rr];
        }
    // pose j: rotation Jr^-1 R_Oj^T;  position -R_A^T R_j [p_Oj]x, dp: R_A^T
    m3_mult(Jr, Oj, T1);
    {
        double Rt[9];
        m3_tmul(RA, Tj, Rt);         // R_A^T R_j
        m3_mul_hat(Rt, Oj + 9, T2);  // R_A^T R_j [p_Oj]x
    }
LVBA_PRIOR_UNROLL
    for (int rr = 0; rr < 3; ++rr)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 3; ++c) {
            Jj[6 * rr + c] = T1[3 * rr + c];
            Jj[6 * rr + 3 + c] = 0.0;
            Jj[6 * (rr + 3) + c] = -T2[3 * rr + c];
            Jj[6 * (rr + 3) + 3 + c] = RA[3 * c + rr];
        }
}

// e = L r (POSITION: the top-left 3 x 3 of L, e[3..5] = 0); returns 1/2 |e|^2
LVBA_HD double prior_whiten(int kind, const double *L, const double *r, double *e)
{
    const int m = kind == PRIOR_POSITION ? 3 : 6;
    double s = 0.0;
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 6; ++a) {
        double v = 0.0;
LVBA_PRIOR_UNROLL
        for (int b = 0; b < 6; ++b)
            if (a < m && b < m) v += L[6 * a + b] * r[b];
        e[a] = v;
        s += v * v;
    }
    return 0.5 * s;
}

// W = L J (row-major 6 x 6; POSITION: rows / columns of L beyond 3 are not read, rows 3..5 of W are zero)
LVBA_HD void prior_whiten_jac(int kind, const double *L, const double *J, double *W)
{
    const int m = kind == PRIOR_POSITION ? 3 : 6;
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 6; ++a)
LVBA_PRIOR_UNROLL
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
LVBA_PRIOR_UNROLL
            for (int b = 0; b < 6; ++b)
                if (a < m && b < m) v += L[6 * a + b] * J[6 * b + c];
            W[6 * a + c] = v;
        }
}

// lin record of an edge, PL_LIN doubles: [0] unused, [1..6] W_i^T e, [7..12] W_j^T e, [13..48] W_i^T W_i, [49..84] W_j^T W_j,
// [85..120] cross block, 6 x 6 blocks in the store's element order (column-major: [c * 6 + r])
enum { PL_GI = 1, PL_GJ = 7, PL_HII = 13, PL_HJJ = 49, PL_HX = 85, PL_LIN = 128 };

// The products of a whitened block W (row-major 6 x 6) that a lin record keeps:
// o[g0 + c] = (W^T e)(c), o[h0 + 6 c + r] = (W^T W)(r, c).  Every element is its own sum over a = 0..5, from 0.0.
LVBA_HD void prior_products(const double *W, const double *e, double *o, int g0, int h0)
{
LVBA_PRIOR_UNROLL
    for (int c = 0; c < 6; ++c) {
        double s = 0.0;
LVBA_PRIOR_UNROLL
        for (int a = 0; a < 6; ++a) s += W[6 * a + c] * e[a];
        o[g0 + c] = s;
    }
LVBA_PRIOR_UNROLL
    for (int c = 0; c < 6; ++c)
LVBA_PRIOR_UNROLL
        for (int r = 0; r < 6; ++r) {
            double s = 0.0;
LVBA_PRIOR_UNROLL
            for (int a = 0; a < 6; ++a) s += W[6 * a + r] * W[6 * a + c];
            o[h0 + 6 * c + r] = s;
        }
}

// The cross block (W_i^T W_j)(r, c) of a RELATIVE prior, block (i, j), into o[x0 ..].  The store keeps (max, min) in solver order;
// flip: j comes after i, the block kept is (j, i), the transpose.
LVBA_HD void prior_cross(const double *Wi, const double *Wj, bool flip, double *o, int x0)
{
LVBA_PRIOR_UNROLL
    for (int c = 0; c < 6; ++c)
LVBA_PRIOR_UNROLL
        for (int r = 0; r < 6; ++r) {
            double x = 0.0;
LVBA_PRIOR_UNROLL
            for (int a = 0; a < 6; ++a) x += Wi[6 * a + r] * Wj[6 * a + c];
            o[x0 + (flip ? 6 * r + c : 6 * c + r)] = x;
        }
}

// T [12] = pose I of poses [n][12]
LVBA_HD void prior_load_pose(const double *poses, int32_t I, double *T)
{
LVBA_PRIOR_UNROLL
    for (int a = 0; a < 12; ++a) T[a] = poses[12 * (int64_t)I + a];
}

// One edge (record fields meas, oi, oj, L) at the poses Ti, Tj (Tj unused unless RELATIVE): e = L r (6; POSITION: e[3..5] = 0),
// returns 1/2 |e|^2; if jac, Wi / Wj = L dr/dd_i, L dr/dd_j, row-major 6 x 6 (Wj: RELATIVE only).  (jac is a flag, not a test
// of Wi against NULL, for prior_raw's reason.)
LVBA_HD double prior_eval(int kind, const double *meas, const double *oi, const double *oj, const double *L, const double *Ti,
                          const double *Tj, double *e, bool jac, double *Wi, double *Wj)
{
    double r[6], Ji[36], Jj[36];
    prior_raw(kind, meas, Ti, oi, Tj, oj, r, jac, Ji, Jj);
    const double cost = prior_whiten(kind, L, r, e);
    if (jac) {
        prior_whiten_jac(kind, L, Ji, Wi);
        if (kind == PRIOR_RELATIVE) prior_whiten_jac(kind, L, Jj, Wj);
    }
    return cost;
}

// The lin record o [PL_LIN] of an edge from e and its whitened blocks (Wj, flip: RELATIVE only; no other kind writes the j ranges)
LVBA_HD void prior_record(int kind, const double *e, const double *Wi, const double *Wj, bool flip, double *o)
{
    prior_products(Wi, e, o, PL_GI, PL_HII);
    if (kind != PRIOR_RELATIVE) return;
    prior_products(Wj, e, o, PL_GJ, PL_HJJ);
    prior_cross(Wi, Wj, flip, o, PL_HX);
}

#if defined(__HIPCC__)
// Fixed-order sums of NV values per lane over the whole grid (64-lane workgroups, part [gridDim.x][NV]): a tree over the lanes of
// each workgroup, then the workgroup that finishes last (a ticket counter, the only atomic) sums the workgroups' shares in index
// order, writes (or, add, adds) the totals to out[i][0] (an out[i] may be NULL) and resets the ticket for the next launch on the
// stream.  The bytes do not change run to run.
template <int NV>
__device__ void prior_grid_sum(const double (&v)[NV], double *__restrict__ part, unsigned *__restrict__ ticket, double *const (&out)[NV],
                               bool add)
{
    __shared__ double red[NV][64];
    __shared__ int last;
    auto tree = [&]() {
        __syncthreads();
        for (int w = 32; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
#pragma unroll
                for (int i = 0; i < NV; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
            }
            __syncthreads();
        }
    };
#pragma unroll
    for (int i = 0; i < NV; ++i) red[i][threadIdx.x] = v[i];
    tree();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) part[NV * blockIdx.x + i] = red[i][0];
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double s[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += 64) {
#pragma unroll
        for (int i = 0; i < NV; ++i) s[i] += __builtin_nontemporal_load(part + NV * b + i);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) red[i][threadIdx.x] = s[i];
    tree();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (out[i]) out[i][0] = add ? out[i][0] + red[i][0] : red[i][0];
        *ticket = 0u;
    }
}
#endif

} // namespace lvba
