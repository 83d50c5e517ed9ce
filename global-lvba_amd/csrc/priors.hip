// priors.hip -- the pose priors of the LiDAR bundle adjustment (lvba_balm_set_priors; the model is in prior_device.h).
//   prior_lin_kernel      one lane per prior: e = L r and the whitened Jacobian blocks at the solver-order poses (prior_eval), and
//                         their lin record (prior_record), both of prior_device.h; writes per prior
//                         J_i^T e, J_j^T e and the 6 x 6 products J_i^T J_i, J_j^T J_j, J_i^T J_j (the last oriented for the lower
//                         block store: transposed when the solver puts i before j), and adds the prior cost to the evaluation's
//   prior_scatter_kernel  every target element of the block store and of g sums its contributions in the fixed order of a CSR table
//                         built on the host.  No atomics on data: the bytes do not change run to run.
//   prior_cost_kernel     the cost alone (the LM's trial point; prior_eval without Jacobians), one lane per prior, summed like
//                         the evaluation's
// Both sums run in the fixed order of prior_grid_sum (prior_device.h).
// An evaluation is 2 launches, a trial cost 1; a handle without priors launches none of them.
#include <hip/hip_runtime.h>

#include "lvba_internal.h"

namespace lvba {

#define PRIOR_WG 256

// prior k's lin record (PL_*), returns its cost.  (kind is a constant at each call site: every array stays in registers)
__device__ __forceinline__ double prior_lin_one(const int kind, const PriorRec &p, const double *__restrict__ poses, double *__restrict__ o)
{
    double Ti[12], Tj[12], e[6], Wi[36], Wj[36];
    prior_load_pose(poses, p.I, Ti);
    if (kind == PRIOR_RELATIVE) prior_load_pose(poses, p.J, Tj);
    const double cost = prior_eval(kind, p.meas, p.oi, p.oj, p.L, Ti, Tj, e, true, Wi, Wj);
    prior_record(kind, e, Wi, Wj, p.flip, o);
    return cost;
}

__global__ __launch_bounds__(64) void prior_lin_kernel(const PriorRec *__restrict__ pr, int32_t n, const double *__restrict__ poses,
                                                       double *__restrict__ lin, double *__restrict__ part, unsigned *__restrict__ ticket,
                                                       double *__restrict__ scal)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c = 0.0;
    if (k < n) {
        const PriorRec &p = pr[k];
        double *o = lin + PL_LIN * (int64_t)k;
        if (p.kind == PRIOR_POSE) c = prior_lin_one(PRIOR_POSE, p, poses, o);
        else if (p.kind == PRIOR_POSITION) c = prior_lin_one(PRIOR_POSITION, p, poses, o);
        else c = prior_lin_one(PRIOR_RELATIVE, p, poses, o);
    }
    prior_grid_sum<1>({c}, part, ticket, {scal}, true);
}

__global__ __launch_bounds__(64) void prior_cost_kernel(const PriorRec *__restrict__ pr, int32_t n, const double *__restrict__ poses,
                                                        double *__restrict__ part, unsigned *__restrict__ ticket, double *__restrict__ out,
                                                        double *__restrict__ e_out)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c = 0.0;
    if (k < n) {
        const PriorRec &p = pr[k];
        double Ti[12], Tj[12], e[6];
        prior_load_pose(poses, p.I, Ti);
        if (p.kind == PRIOR_RELATIVE) prior_load_pose(poses, p.J, Tj);
        c = prior_eval(p.kind, p.meas, p.oi, p.oj, p.L, Ti, Tj, e, false, nullptr, nullptr);
        if (e_out) {
LVBA_PRIOR_UNROLL
            for (int a = 0; a < 6; ++a) e_out[6 * (int64_t)k + a] = e[a];
        }
    }
    prior_grid_sum<1>({c}, part, ticket, {out}, true);
}

__global__ __launch_bounds__(PRIOR_WG) void prior_scatter_kernel(PriorDev d, double *__restrict__ Hblk, double *__restrict__ g)
{
    const int64_t t = (int64_t)blockIdx.x * PRIOR_WG + threadIdx.x;
    if (t < 36 * d.n_hblk) {
        const int64_t b = t / 36;
        const int el = (int)(t - 36 * b);
        const int mode = d.hmode[b];
        if ((mode & 2) && (el % 6) < (el / 6)) return; // diagonal block: only the lower triangle is stored
        double *dst = Hblk + d.hslot[b] * 36 + el;
        double s = (mode & 1) ? 0.0 : *dst;
        for (int32_t q = d.hoff[b]; q < d.hoff[b + 1]; ++q) {
            const int32_t src = d.hsrc[q], k = src >> 2, piece = src & 3;
            s += d.lin[PL_LIN * (int64_t)k + (piece == 0 ? PL_HII : piece == 1 ? PL_HJJ : PL_HX) + el];
        }
        *dst = s;
        return;
    }
    const int64_t u = t - 36 * d.n_hblk;
    if (u >= 6 * (int64_t)d.n_g) return;
    const int64_t b = u / 6;
    const int el = (int)(u - 6 * b);
    double *dst = g + 6 * (int64_t)d.gpose[b] + el;
    double s = *dst;
    for (int32_t q = d.goff[b]; q < d.goff[b + 1]; ++q) {
        const int32_t src = d.gsrc[q], k = src >> 2, piece = src & 3;
        s += d.lin[PL_LIN * (int64_t)k + (piece == 0 ? PL_GI : PL_GJ) + el];
    }
    *dst = s;
}

__global__ void prior_zero_slots_kernel(double *__restrict__ Hblk, const int64_t *__restrict__ slot, int64_t n)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < 36 * n) Hblk[slot[t / 36] * 36 + t % 36] = 0.0;
}

void launch_prior_scatter(const PriorDev &d, double *Hblk, double *g, hipStream_t s)
{
    if (d.n <= 0) return;
    const int64_t work = 36 * d.n_hblk + 6 * (int64_t)d.n_g;
    hipLaunchKernelGGL(prior_scatter_kernel, dim3((unsigned)((work + PRIOR_WG - 1) / PRIOR_WG)), dim3(PRIOR_WG), 0, s, d, Hblk, g);
}

void launch_prior_eval(const PriorDev &d, const double *poses, double *Hblk, double *g, double *scal, hipStream_t s)
{
    if (d.n <= 0) return;
    hipLaunchKernelGGL(prior_lin_kernel, dim3((unsigned)((d.n + 63) / 64)), dim3(64), 0, s, d.pr, d.n, poses, d.lin, d.part, d.ticket, scal);
    launch_prior_scatter(d, Hblk, g, s);
}

void launch_prior_cost(const PriorDev &d, const double *poses, double *out, double *e_out, hipStream_t s)
{
    if (d.n <= 0) return;
    hipLaunchKernelGGL(prior_cost_kernel, dim3((unsigned)((d.n + 63) / 64)), dim3(64), 0, s, d.pr, d.n, poses, d.part, d.ticket, out, e_out);
}

void launch_prior_zero_slots(double *Hblk, const int64_t *slot, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(prior_zero_slots_kernel, dim3((unsigned)((36 * n + 255) / 256)), dim3(256), 0, s, Hblk, slot, n);
}

} // namespace lvba
