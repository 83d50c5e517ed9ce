// visual_priors.hip -- the camera pose priors of the visual bundle adjustment (lvba_visual_set_priors; the model is in
// visual_prior_device.h).  A prior is one more residual block on one or two cameras, outside the losses:
//   vprior_lin_kernel     one lane per prior: e = L r and the whitened Jacobian blocks W_i, W_j in the visual tangent at the
//                         solver-order cameras, columns scaled by the Jacobi scaling (or not: iteration 0, which derives it);
//                         writes the LiDAR stage's lin record (prior_record, prior_device.h) -- W_i^T e, W_j^T e, W_i^T W_i,
//                         W_j^T W_j, the cross block oriented for the lower block store; the diagonals of the two squares are the
//                         squared column norms -- and
//                         adds sum |e|^2 to the evaluation's.  The constant camera's columns are zero.
//   prior_scatter_kernel  (priors.hip, shared) the records into the block store and the reduced right-hand side
//   vprior_cam_kernel     the records into the per-camera sums the LM diagonal, the gradient max and the Jacobi scaling are
//                         derived from, in the fixed order of the same host-built CSR table
//   vprior_trial_kernel   one launch per LM iteration: sum |e|^2 at the trial point and the priors' share -(W d).(e + W d / 2)
//                         of the model cost change for the camera step d
// The grid-wide sums (two values per lane) run in the fixed order of prior_grid_sum (prior_device.h).
#include <hip/hip_runtime.h>

#include "lvba_internal.h"
#include "visual_prior_device.h"

namespace lvba {

__device__ __forceinline__ void vprior_load_cam(const double *__restrict__ qc, const double *__restrict__ tc, int32_t I, double *q, double *t)
{
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = qc[4 * (int64_t)I + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = tc[3 * (int64_t)I + a];
}

// column scales of camera I's tangent: 0 for the constant camera, the Jacobi scaling when there is one, else 1
__device__ __forceinline__ void vprior_scales(const double *__restrict__ sc_cam, int32_t I, int32_t fixed_cam, double *sc)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) sc[c] = I == fixed_cam ? 0.0 : (sc_cam ? sc_cam[6 * (int64_t)I + c] : 1.0);
}

// one prior's lin record; returns |e|^2.  (kind is a constant at each call site, as in priors.hip: every array stays in registers)
__device__ __forceinline__ double vprior_lin_one(const int kind, const PriorRec &p, int32_t fixed_cam, const double *__restrict__ qc,
                                                 const double *__restrict__ tc, const double *__restrict__ sc_cam, double *__restrict__ o)
{
    double qi[4], ti[3], qj[4], tj[3], e[6], Wi[36], Wj[36], sc[6];
    vprior_load_cam(qc, tc, p.I, qi, ti);
    vprior_load_cam(qc, tc, kind == PRIOR_RELATIVE ? p.J : p.I, qj, tj);
    const double c2 = 2.0 * vprior_eval(kind, p.meas, p.oi, p.oj, p.L, qi, ti, qj, tj, e, true, Wi, Wj);
    if (kind == PRIOR_RELATIVE) { // (j before i: the order that needs the fewest registers)
        vprior_scales(sc_cam, p.J, fixed_cam, sc);
#pragma unroll
        for (int a = 0; a < 36; ++a) Wj[a] *= sc[a % 6];
    }
    vprior_scales(sc_cam, p.I, fixed_cam, sc);
#pragma unroll
    for (int a = 0; a < 36; ++a) Wi[a] *= sc[a % 6];
    prior_record(kind, e, Wi, Wj, p.flip, o);
    return c2;
}

__global__ __launch_bounds__(64) void vprior_lin_kernel(const PriorRec *__restrict__ pr, int32_t n, int32_t fixed_cam,
                                                        const double *__restrict__ qc, const double *__restrict__ tc,
                                                        const double *__restrict__ sc_cam, double *__restrict__ lin,
                                                        double *__restrict__ part, unsigned *__restrict__ ticket, double *__restrict__ scal0)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c2 = 0.0;
    if (k < n) {
        const PriorRec &p = pr[k];
        double *o = lin + PL_LIN * (int64_t)k;
        if (p.kind == PRIOR_POSE) c2 = vprior_lin_one(PRIOR_POSE, p, fixed_cam, qc, tc, sc_cam, o);
        else if (p.kind == PRIOR_POSITION) c2 = vprior_lin_one(PRIOR_POSITION, p, fixed_cam, qc, tc, sc_cam, o);
        else c2 = vprior_lin_one(PRIOR_RELATIVE, p, fixed_cam, qc, tc, sc_cam, o);
    }
    prior_grid_sum<2>({c2, 0.0}, part, ticket, {scal0, nullptr}, true);
}

// per camera with priors (the g table: piece 0 = the prior's camera i, 1 = its camera j): diag [6 I + el] += sum of the squared
// column norms, and when grad, grad [6 I + el] += sum of W^T e
__global__ __launch_bounds__(256) void vprior_cam_kernel(PriorDev d, double *__restrict__ diag, double *__restrict__ grad)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= 6 * (int64_t)d.n_g) return;
    const int64_t b = u / 6;
    const int el = (int)(u - 6 * b);
    const int64_t dst = 6 * (int64_t)d.gpose[b] + el;
    double sd = diag[dst], sg = grad ? grad[dst] : 0.0;
    for (int32_t q = d.goff[b]; q < d.goff[b + 1]; ++q) {
        const int32_t src = d.gsrc[q], k = src >> 2, piece = src & 3;
        const double *o = d.lin + PL_LIN * (int64_t)k;
        sd += o[(piece == 0 ? PL_HII : PL_HJJ) + 7 * el];
        sg += o[(piece == 0 ? PL_GI : PL_GJ) + el];
    }
    diag[dst] = sd;
    if (grad) grad[dst] = sg;
}

// one prior at the trial point (qc2, tc2): |e|^2 (returned, e -> e_out) and, with a step, its share of the model cost change
__device__ __forceinline__ double vprior_trial_one(const int kind, const PriorRec &p, int32_t fixed_cam, const double *__restrict__ qc,
                                                   const double *__restrict__ tc, const double *__restrict__ step_c,
                                                   const double *__restrict__ sc_cam, const double *__restrict__ qc2,
                                                   const double *__restrict__ tc2, double *e, double *mc)
{
    const int32_t J = kind == PRIOR_RELATIVE ? p.J : p.I;
    double qi[4], ti[3], qj[4], tj[3];
    if (step_c) { // the model at the linearisation point: m = W_i d_i + W_j d_j in the scaled variables
        double Wi[36], Wj[36], sc[6], m[6];
        vprior_load_cam(qc, tc, p.I, qi, ti);
        vprior_load_cam(qc, tc, J, qj, tj);
        vprior_eval(kind, p.meas, p.oi, p.oj, p.L, qi, ti, qj, tj, e, true, Wi, Wj);
        vprior_scales(sc_cam, p.I, fixed_cam, sc);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) s += Wi[6 * a + c] * (sc[c] * step_c[6 * (int64_t)p.I + c]);
            m[a] = s;
        }
        if (kind == PRIOR_RELATIVE) {
            vprior_scales(sc_cam, J, fixed_cam, sc);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) s += Wj[6 * a + c] * (sc[c] * step_c[6 * (int64_t)J + c]);
                m[a] += s;
            }
        }
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) v -= m[a] * (e[a] + 0.5 * m[a]);
        *mc = v;
    }
    vprior_load_cam(qc2, tc2, p.I, qi, ti);
    vprior_load_cam(qc2, tc2, J, qj, tj);
    return 2.0 * vprior_eval(kind, p.meas, p.oi, p.oj, p.L, qi, ti, qj, tj, e, false, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void vprior_trial_kernel(const PriorRec *__restrict__ pr, int32_t n, int32_t fixed_cam,
                                                          const double *__restrict__ qc, const double *__restrict__ tc,
                                                          const double *__restrict__ step_c, const double *__restrict__ sc_cam,
                                                          const double *__restrict__ qc2, const double *__restrict__ tc2,
                                                          double *__restrict__ part, unsigned *__restrict__ ticket,
                                                          double *__restrict__ out_cost, double *__restrict__ out_model, bool add,
                                                          double *__restrict__ e_out)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c2 = 0.0, mc = 0.0;
    if (k < n) {
        const PriorRec &p = pr[k];
        double e[6];
        if (p.kind == PRIOR_POSE) c2 = vprior_trial_one(PRIOR_POSE, p, fixed_cam, qc, tc, step_c, sc_cam, qc2, tc2, e, &mc);
        else if (p.kind == PRIOR_POSITION) c2 = vprior_trial_one(PRIOR_POSITION, p, fixed_cam, qc, tc, step_c, sc_cam, qc2, tc2, e, &mc);
        else c2 = vprior_trial_one(PRIOR_RELATIVE, p, fixed_cam, qc, tc, step_c, sc_cam, qc2, tc2, e, &mc);
        if (e_out) {
#pragma unroll
            for (int a = 0; a < 6; ++a) e_out[6 * (int64_t)k + a] = e[a];
        }
    }
    prior_grid_sum<2>({c2, mc}, part, ticket, {out_cost, out_model}, add);
}

static inline unsigned vprior_grid(int32_t n) { return (unsigned)((n + 63) / 64); }

static void vprior_launch_cam(const PriorDev &t, double *diag, double *grad, hipStream_t s)
{
    hipLaunchKernelGGL(vprior_cam_kernel, dim3((unsigned)((6 * (int64_t)t.n_g + 255) / 256)), dim3(256), 0, s, t, diag, grad);
}

void vprior_launch_lin0(const VisPriorDev &d, const double *qc, const double *tc, double *scal0, hipStream_t s)
{
    const PriorDev &t = d.tab;
    if (t.n <= 0 || !d.active) return;
    hipLaunchKernelGGL(vprior_lin_kernel, dim3(vprior_grid(t.n)), dim3(64), 0, s, t.pr, t.n, d.fixed_cam, qc, tc, (const double *)nullptr,
                       t.lin, t.part, t.ticket, scal0);
}

void vprior_launch_colsum_add(const VisPriorDev &d, double *colsum, hipStream_t s)
{
    if (d.tab.n <= 0 || !d.active) return;
    vprior_launch_cam(d.tab, colsum, nullptr, s);
}

void vprior_launch_eval(const VisPriorDev &d, const double *qc, const double *tc, const double *sc_cam, int32_t M, double *Hblk,
                        double *g, double *camsum, hipStream_t s)
{
    const PriorDev &t = d.tab;
    if (t.n <= 0 || !d.active) return;
    hipLaunchKernelGGL(vprior_lin_kernel, dim3(vprior_grid(t.n)), dim3(64), 0, s, t.pr, t.n, d.fixed_cam, qc, tc, sc_cam, t.lin, t.part,
                       t.ticket, (double *)nullptr);
    launch_prior_scatter(t, Hblk, g, s);
    vprior_launch_cam(t, camsum, camsum + 6 * (int64_t)M, s);
}

void vprior_launch_trial(const VisPriorDev &d, const double *qc, const double *tc, const double *step_c, const double *sc_cam,
                         const double *qc2, const double *tc2, double *out_cost, double *out_model, bool add, double *e_out,
                         hipStream_t s)
{
    const PriorDev &t = d.tab;
    if (t.n <= 0 || !d.active) return;
    hipLaunchKernelGGL(vprior_trial_kernel, dim3(vprior_grid(t.n)), dim3(64), 0, s, t.pr, t.n, d.fixed_cam, qc, tc, step_c, sc_cam, qc2,
                       tc2, t.part, t.ticket, out_cost, out_model, add, e_out);
}

} // namespace lvba
