// palign_device.h -- scalar pieces of the photometric camera alignment (palign.hip; the rule is in include/lvba_hip.h, DESIGN.md
// §10q): the sample of a point with its bilinear gradient, the projection's Jacobian, a channel's residual, row and weight, the
// sums, the damped 6 x 6 solve and the per-image Levenberg-Marquardt step.  Host/device-neutral, like photo_device.h;
// tests/palign_check.cpp compiles it for the host.  All floating-point work is fp64, every expression rounds in the order written
// here, and the including file is built without floating-point contraction: a sample's residuals, rows and weights are the same
// bits under g++, numpy and gfx950 (+, -, *, / and sqrt only with the trivial and the Huber loss).  The sums over the samples are
// a tree on the device and are held to the summation bound instead.
//   Sample of X at (R, t): photo_locate, photo_tap and photo_mix_channel of photo_device.h, unchanged -- the same (u, v), a, b,
//   texels and c16 as the fusion's -- and from the same four texels, per channel k, the gradient in grey levels per pixel
//     gu_k = ((256 - b)(t10 - t00) + b (t11 - t01)) / 256,   gv_k = ((256 - a)(t01 - t00) + a (t11 - t10)) / 256
//   Residual r_k = (c16_k - ref16_k) / 256.  Left perturbation R <- (I + [om]x) R, t <- t + om x t + up, so Xc <- Xc + om x Xc + up:
//   with Jpi the 2 x 3 Jacobian of trk_project_cam at Xc and q_k = gu_k Jpi[0] + gv_k Jpi[1] the row of channel k is (Xc x q_k, q_k).
//   s = r_k^2, rho = loss_eval(s): weight rho', H += rho' J^T J, g += rho' J^T r, cost += rho / 2.
#pragma once
#include <math.h>
#include <stdint.h>
#include "visual_loss.h"
#include "photo_device.h"
#include "resect_device.h"

namespace lvba {

constexpr int PAL_NS = 31;                  // sums per image: H upper triangle by row (21), g (6), cost, samples, sum r^2, sum rho'
constexpr int PAL_G0 = 21, PAL_COST = 27, PAL_CNT = 28, PAL_SSQ = 29, PAL_SW = 30;
constexpr int PAL_BLOCK = 256;              // lanes of a linearisation workgroup
constexpr int PAL_CHUNK = 4096;             // points of a workgroup: lane l takes the points chunk * PAL_CHUNK + l + k * PAL_BLOCK
constexpr double PAL_LAMBDA0 = 1e-3, PAL_LAMBDA_MIN = 1e-9, PAL_DIAG_FLOOR = 1e-12;
// image states (the LVBA_PALIGN_* values of include/lvba_hip.h; RUNNING is internal)
enum { PAL_CONVERGED = 0, PAL_MAX_ITERATIONS = 1, PAL_TOO_FEW = 2, PAL_DEGENERATE = 3, PAL_OUT_OF_BOUNDS = 4, PAL_RUNNING = -1 };

struct PalParams { // lvba_palign_opts on the device
    double loss_scale, eps_rot, eps_trans;
    double max_chord_sq;     // |R - R0|_F^2 of a rotation by max_rotation: 8 sin^2(max_rotation / 2)
    double max_translation;
    int32_t loss_kind, min_samples, max_iterations, pad;
};

struct PalState { // an image's iteration: what the linearisation reads (status, Rt, tt) and what the step keeps
    int32_t status, passes, accepted, pad;
    double lambda;
    double R0[9], t0[3];     // the initial pose
    double R[9], t[3];       // the current pose: the initial one, then the last accepted trial
    double Rt[9], tt[3];     // the pose of the next linearisation
    double d[6];             // the step that led to (Rt, tt)
    double cur[PAL_NS];      // the sums at (R, t)
    double first[PAL_NS];    // the sums at (R0, t0)
};

// the number of workgroups the n points of an image are summed by: a function of n alone
LVBA_TRK_FN int64_t pal_chunks(int64_t n) { return n <= PAL_CHUNK ? 1 : (n + PAL_CHUNK - 1) / PAL_CHUNK; }

// the gradient's integer numerators of channel k, in 1/256 grey level per pixel: |.| <= 255 * 256
LVBA_TRK_FN void pal_gradient_num(const PhotoTap &p, int k, int32_t &nu, int32_t &nv)
{
    const int32_t t00 = photo_byte(p.t00, k), t10 = photo_byte(p.t10, k), t01 = photo_byte(p.t01, k), t11 = photo_byte(p.t11, k);
    nu = (256 - p.b) * (t10 - t00) + p.b * (t11 - t01);
    nv = (256 - p.a) * (t01 - t00) + p.a * (t11 - t10);
}

// channel k of a sample: its colour c16 and its gradient (gu, gv) in grey levels per pixel
struct PalColour { int32_t c16; double gu, gv; };
LVBA_TRK_FN PalColour pal_colour(const PhotoTap &p, int k)
{
    int32_t nu, nv;
    pal_gradient_num(p, k, nu, nv);
    PalColour c;
    c.c16 = photo_mix_channel(p, k);
    c.gu = (double)nu / 256.0;
    c.gv = (double)nv / 256.0;
    return c;
}

// Xc = R X + t, each row as trk_project writes it
LVBA_TRK_FN void pal_camera_point(const double *__restrict__ R, const double *__restrict__ t, const double *__restrict__ X, double *__restrict__ Xc)
{
    Xc[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    Xc[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    Xc[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
}

// Ju, Jv [3]: the derivatives of trk_project_cam's (u, v) by Xc, Brown-Conrady included (Xc_z > 0: the point was sampled).
//   x = Xc_x / Xc_z, y likewise; radial = 1 + k1 r2 + k2 r2^2, dr = d radial / d r2 = k1 + 2 k2 r2
//   d xd / dx = radial + 2 x^2 dr + 2 p1 y + 6 p2 x     d xd / dy = d yd / dx = 2 x y dr + 2 p1 x + 2 p2 y
//   d yd / dy = radial + 2 y^2 dr + 6 p1 y + 2 p2 x     dx / dXc = (1, 0, -x) / Xc_z,  dy / dXc = (0, 1, -y) / Xc_z
LVBA_TRK_FN void pal_jpi(const TrkIntr &c, const double *__restrict__ Xc, double *__restrict__ Ju, double *__restrict__ Jv)
{
    const double iz = 1.0 / Xc[2];
    const double x = Xc[0] / Xc[2], y = Xc[1] / Xc[2];
    const double r2 = x * x + y * y, r4 = r2 * r2;
    const double radial = 1.0 + c.k1 * r2 + c.k2 * r4;
    const double dr = c.k1 + 2.0 * c.k2 * r2;
    const double a00 = (radial + 2.0 * (x * x) * dr) + (2.0 * c.p1 * y + 6.0 * c.p2 * x);
    const double a01 = 2.0 * (x * y) * dr + (2.0 * c.p1 * x + 2.0 * c.p2 * y);
    const double a11 = (radial + 2.0 * (y * y) * dr) + (6.0 * c.p1 * y + 2.0 * c.p2 * x);
    Ju[0] = c.fx * (a00 * iz); Ju[1] = c.fx * (a01 * iz); Ju[2] = -(c.fx * ((a00 * x + a01 * y) * iz));
    Jv[0] = c.fy * (a01 * iz); Jv[1] = c.fy * (a11 * iz); Jv[2] = -(c.fy * ((a01 * x + a11 * y) * iz));
}

// a channel's residual r against its reference, its row J [6] in the order (om, up) and rho [3] of its loss
LVBA_TRK_FN void pal_channel(const PalColour &c, uint16_t ref16, const double *__restrict__ Xc, const double *__restrict__ Ju,
                             const double *__restrict__ Jv, int loss_kind, double loss_scale, double &r, double *__restrict__ J,
                             double *__restrict__ rho)
{
    r = (double)(c.c16 - (int32_t)ref16) / 256.0;
    const double q0 = c.gu * Ju[0] + c.gv * Jv[0], q1 = c.gu * Ju[1] + c.gv * Jv[1], q2 = c.gu * Ju[2] + c.gv * Jv[2];
    J[0] = Xc[1] * q2 - Xc[2] * q1;
    J[1] = Xc[2] * q0 - Xc[0] * q2;
    J[2] = Xc[0] * q1 - Xc[1] * q0;
    J[3] = q0; J[4] = q1; J[5] = q2;
    loss_eval(loss_kind, loss_scale, r * r, rho);
}

// a channel's terms into the sums s [PAL_NS] (registers on the device: every index is a constant after unrolling)
LVBA_TRK_FN void pal_accumulate(double r, const double *__restrict__ J, const double *__restrict__ rho, double *__restrict__ s)
{
    const double wt = rho[1];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double wj = wt * J[a];
#pragma unroll
        for (int b = a; b < 6; ++b) s[k++] += wj * J[b];
        s[PAL_G0 + a] += wj * r;
    }
    s[PAL_COST] += 0.5 * rho[0];
    s[PAL_SSQ] += r * r;
    s[PAL_SW] += wt;
}

// One point in one image: its three channels into the sums, one after the other (the loop stays rolled on the device: a channel's
// work is a function of k through shifts alone), and the sample into the count.
template <class Texel>
LVBA_TRK_FN void pal_point(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                           const double *__restrict__ tj, const double *__restrict__ X, const uint16_t *__restrict__ ref16,
                           const PhotoRule &o, int loss_kind, double loss_scale, Texel texel, double *__restrict__ s)
{
    double u, v;
    if (!photo_locate(cam, depth_j, w, h, Rj, tj, X, o, u, v)) return;
    const PhotoTap p = photo_tap(u, v, texel);
    double Xc[3], Ju[3], Jv[3];
    pal_camera_point(Rj, tj, X, Xc);
    pal_jpi(cam, Xc, Ju, Jv);
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        double r, J[6], rho[3];
        pal_channel(pal_colour(p, k), ref16[k], Xc, Ju, Jv, loss_kind, loss_scale, r, J, rho);
        pal_accumulate(r, J, rho, s);
    }
    s[PAL_CNT] += 1.0;
}

// the full symmetric matrix of the 21 upper-triangle sums
LVBA_TRK_FN void pal_expand(const double *s, double *A)
{
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[6 * a + b] = A[6 * b + a] = s[k]; ++k; }
}

// d = -(H + lambda diag(max(H_aa, PAL_DIAG_FLOOR)))^-1 g from the sums s, by LDL^T without pivoting (the matrix is positive definite
// where H is positive semi-definite with a positive diagonal).  false: a pivot that is not > 0, or a step that is not finite.
LVBA_TRK_FN bool pal_solve(const double *s, double lambda, double *d)
{
    double A[36], L[36], D[6], y[6];
    pal_expand(s, A);
    for (int a = 0; a < 6; ++a) {
        const double h = A[7 * a];
        A[7 * a] = h + lambda * (h > PAL_DIAG_FLOOR ? h : PAL_DIAG_FLOOR);
    }
    for (int j = 0; j < 6; ++j) {
        double dj = A[7 * j];
        for (int k = 0; k < j; ++k) dj -= (L[6 * j + k] * L[6 * j + k]) * D[k];
        if (!(dj > 0.0)) return false;
        D[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[6 * i + j];
            for (int k = 0; k < j; ++k) v -= (L[6 * i + k] * L[6 * j + k]) * D[k];
            L[6 * i + j] = v / dj;
        }
    }
    for (int i = 0; i < 6; ++i) {          // L y = -g
        double v = -s[PAL_G0 + i];
        for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
        y[i] = v;
    }
    for (int i = 5; i >= 0; --i) {         // L^T d = D^-1 y
        double v = y[i] / D[i];
        for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * d[k];
        d[i] = v;
    }
    for (int a = 0; a < 6; ++a)
        if (!isfinite(d[a])) return false;
    return true;
}

// (Rn, tn) = the perturbation d = (om, up) applied to (R, t): R <- (I + [om]x) R through a unit quaternion, t <- t + om x t + up
// (resect_step's retraction)
LVBA_TRK_FN void pal_retract(const double *R, const double *t, const double *d, double *Rn, double *tn)
{
    for (int c = 0; c < 3; ++c) {
        Rn[c] = R[c] + (d[1] * R[6 + c] - d[2] * R[3 + c]);
        Rn[3 + c] = R[3 + c] + (d[2] * R[c] - d[0] * R[6 + c]);
        Rn[6 + c] = R[6 + c] + (d[0] * R[3 + c] - d[1] * R[c]);
    }
    tn[0] = t[0] + (d[1] * t[2] - d[2] * t[1]) + d[3];
    tn[1] = t[1] + (d[2] * t[0] - d[0] * t[2]) + d[4];
    tn[2] = t[2] + (d[0] * t[1] - d[1] * t[0]) + d[5];
    resect_orthonormalise(Rn);
}

// is (R, t) further than the bounds from (R0, t0)?  The rotation by the chord |R - R0|_F^2 = 8 sin^2(angle / 2), the translation by
// the camera centres C = -R^T t.
LVBA_TRK_FN bool pal_out_of_bounds(const double *R, const double *t, const double *R0, const double *t0, const PalParams &o)
{
    double chord = 0.0;
    for (int e = 0; e < 9; ++e) chord += (R[e] - R0[e]) * (R[e] - R0[e]);
    double dc = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double C = (R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2], C0 = (R0[c] * t0[0] + R0[3 + c] * t0[1]) + R0[6 + c] * t0[2];
        dc += (C - C0) * (C - C0);
    }
    return !(chord <= o.max_chord_sq) || !(sqrt(dc) <= o.max_translation);
}

LVBA_TRK_FN void pal_state_init(PalState &st, const double *R, const double *t)
{
    st.status = PAL_RUNNING; st.passes = 0; st.accepted = 0; st.pad = 0;
    st.lambda = PAL_LAMBDA0;
    for (int e = 0; e < 9; ++e) st.R0[e] = st.R[e] = st.Rt[e] = R[e];
    for (int e = 0; e < 3; ++e) st.t0[e] = st.t[e] = st.tt[e] = t[e];
    for (int e = 0; e < 6; ++e) st.d[e] = 0.0;
    for (int q = 0; q < PAL_NS; ++q) st.cur[q] = st.first[q] = 0.0;
}

// One pass of an image: s [PAL_NS] are the sums at (st.Rt, st.tt).  The first pass is the linearisation at the initial pose; every
// later one judges the trial: accepted iff it has min_samples samples and its mean cost is below the current one.  Returns the
// image's state; on RUNNING (st.Rt, st.tt) is the next trial.  A pose that is refused, degenerate or out of bounds goes back as it
// came: (st.R, st.t) = (st.R0, st.t0) with the sums of the first pass.
LVBA_TRK_FN int pal_step(const double *s, const PalParams &o, PalState &st)
{
    st.passes += 1;
    const double n = s[PAL_CNT];
    if (st.passes == 1) {
        for (int q = 0; q < PAL_NS; ++q) st.cur[q] = st.first[q] = s[q];
        if (n < (double)o.min_samples) return PAL_TOO_FEW;
    } else {
        const bool accept = n >= (double)o.min_samples && s[PAL_COST] / n < st.cur[PAL_COST] / st.cur[PAL_CNT];
        if (accept) {
            for (int e = 0; e < 9; ++e) st.R[e] = st.Rt[e];
            for (int e = 0; e < 3; ++e) st.t[e] = st.tt[e];
            for (int q = 0; q < PAL_NS; ++q) st.cur[q] = s[q];
            st.accepted += 1;
            const double l = st.lambda / 3.0;
            st.lambda = l > PAL_LAMBDA_MIN ? l : PAL_LAMBDA_MIN;
            if (pal_out_of_bounds(st.R, st.t, st.R0, st.t0, o)) {
                for (int e = 0; e < 9; ++e) st.R[e] = st.R0[e];
                for (int e = 0; e < 3; ++e) st.t[e] = st.t0[e];
                for (int q = 0; q < PAL_NS; ++q) st.cur[q] = st.first[q];
                return PAL_OUT_OF_BOUNDS;
            }
            const double *d = st.d;
            const double dr = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), dt = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
            if (dr <= o.eps_rot && dt <= o.eps_trans) return PAL_CONVERGED;
        } else {
            st.lambda = 4.0 * st.lambda;
        }
    }
    if (st.passes >= o.max_iterations) return PAL_MAX_ITERATIONS;
    bool ok = true;
    for (int a = 0, k = 0; a < 6; k += 6 - a, ++a) ok = ok && st.cur[k] > 0.0;   // the diagonal of H
    if (ok) ok = pal_solve(st.cur, st.lambda, st.d);
    if (!ok) {
        for (int e = 0; e < 9; ++e) st.R[e] = st.R0[e];
        for (int e = 0; e < 3; ++e) st.t[e] = st.t0[e];
        for (int q = 0; q < PAL_NS; ++q) st.cur[q] = st.first[q];
        return PAL_DEGENERATE;
    }
    pal_retract(st.R, st.t, st.d, st.Rt, st.tt);
    return PAL_RUNNING;
}

} // namespace lvba
