// calib.hip -- LiDAR-camera extrinsic refinement from depth-lifted matches: Gauss-Newton on the six parameters of T_cam<-imu over
// the records of all image pairs, for a batch of initial extrinsics (jobs) over the same records, in lock-step.  The pair
// transform, the per-record rule, the partition and the per-job step are calib_device.h (also compiled for the host by the tests);
// definitions in include/lvba_hip.h and DESIGN.md §10o.  The second half of the file is the same iteration with the camera-LiDAR
// time offset as a seventh parameter (lvba_calib_*_td; calib_td_device.h).
//
// Device design -- the registration's (register.hip) --, one launch per call, then per iteration two and one word read by the host:
//   calib_prepare_kernel    a thread per pair: its transform A = T_imu_a<-imu_b [12]; a thread per record: its target pixel
//                           undistorted once, NaN where the record is unusable.
//   calib_linearize_kernel  grid (workgroups, jobs), nb = cal_blocks(n) workgroups -- a function of the record count alone, so a
//                           job's bytes do not depend on what else is in the batch.  Lane l of workgroup b takes the records
//                           b * 256 + l + k * nb * 256: coalesced loads of 4 + 16 + 24 bytes per record; the pair's transform is
//                           fetched by index (records come grouped by pair: neighbouring lanes share it, and the table stays in
//                           L2).  The extrinsic is uniform and stays in scalar registers, the CAL_NS sums in vector registers.
//                           Then the fixed tree of wave_ops.h, the four wavefronts' shares added in index order through LDS, one
//                           partial [CAL_NS] per workgroup.  No atomics: the bytes do not change run to run.
//   calib_step_kernel       one wavefront per job: lane q adds the job's partials of sum q in index order; lane 0 takes the
//                           eigen-decomposition of H (cyclic Jacobi, 6 x 6, in LDS), decides the held set and the job's state and
//                           retracts the extrinsic in place.  A job that goes on sets the iteration's word in the host's pinned
//                           memory; the lanes of a finished job return at once in both kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "image_set.h"
#include "wave_ops.h"
#include "calib_device.h"
#include "calib_td_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

static_assert(LVBA_CALIB_CONVERGED == CAL_CONVERGED && LVBA_CALIB_MAX_ITERATIONS == CAL_MAX_ITERATIONS &&
              LVBA_CALIB_TOO_FEW_RECORDS == CAL_TOO_FEW && LVBA_CALIB_DEGENERATE == CAL_DEGENERATE &&
              LVBA_CALIB_TD_OUT_OF_RANGE == CAL_TD_OUT_OF_RANGE && LVBA_CALIB_TD_SUMS == CAL_TD_NS, "calibration states");
static_assert(CAL_BLOCK == 256, "the linearisation adds four wavefronts' shares");

namespace {

// pairT [n_pairs][12], xy [n][2]
__global__ __launch_bounds__(256) void calib_prepare_kernel(int64_t n, int32_t n_pairs, const double *__restrict__ poses,
                                                            const int32_t *__restrict__ img_a, const int32_t *__restrict__ img_b,
                                                            const float *__restrict__ uv, const double *__restrict__ Xb, TrkIntr cam,
                                                            double *__restrict__ pairT, double *__restrict__ xy)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pairs) {
        double A[12];
        cal_pair(poses + 12 * (int64_t)img_a[i], poses + 12 * (int64_t)img_b[i], A);
#pragma unroll
        for (int k = 0; k < 12; ++k) pairT[12 * i + k] = A[k];
    }
    if (i < n) {
        const double X[3] = {Xb[3 * i], Xb[3 * i + 1], Xb[3 * i + 2]};
        double x, y;
        cal_target(cam, uv[2 * i], uv[2 * i + 1], X, x, y);
        xy[2 * i] = x; xy[2 * i + 1] = y;
    }
}

// ext [jobs][12] = (R row-major | t); part [jobs][gridDim.x][CAL_NS]
__global__ __launch_bounds__(CAL_BLOCK) void calib_linearize_kernel(int64_t n, const int32_t *__restrict__ pair, const double *__restrict__ xy,
                                                                    const double *__restrict__ Xb, const double *__restrict__ pairT,
                                                                    const double *__restrict__ ext, const CalResult *__restrict__ res,
                                                                    const CalParams o, double *__restrict__ part)
{
    __shared__ double red[CAL_BLOCK / 64][CAL_NS];
    const int job = blockIdx.y;
    if (res[job].status != CAL_RUNNING) return;
    const int nb = cal_blocks(n);
    if ((int)blockIdx.x >= nb) return;
    double T[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) T[a] = ext[12 * (int64_t)job + a];
    double s[CAL_NS];
#pragma unroll
    for (int q = 0; q < CAL_NS; ++q) s[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * CAL_BLOCK + threadIdx.x; i < n; i += (int64_t)nb * CAL_BLOCK) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        if (!(x == x && y == y)) continue;
        const double X[3] = {Xb[3 * i], Xb[3 * i + 1], Xb[3 * i + 2]};
        const double *__restrict__ Ap = pairT + 12 * (int64_t)pair[i];
        double A[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) A[a] = Ap[a];
        cal_record(T, T + 9, A, x, y, X, o, s);
    }
#pragma unroll
    for (int q = 0; q < CAL_NS; ++q) s[q] = wave_sum_to_lane63(s[q]); // (a lane without a source adds 0.0)
    // per component, from lane 63, for CAL_NS threads to finish (as reg_linearize_kernel does)
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < CAL_NS; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < CAL_NS) {
        const int q = threadIdx.x;
        part[((int64_t)job * gridDim.x + blockIdx.x) * CAL_NS + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// nb: the linearisation's gridDim.x = cal_blocks(n).  sums_only: lvba_calib_linearize (no step).  may_step: 0 at the evaluation
// that follows the last allowed step.  sums [jobs][CAL_NS] keeps the sums of the job's last linearisation.  flag: the host's word of
// this iteration, set by every job that goes on.
__global__ __launch_bounds__(64) void calib_step_kernel(int nb, const double *__restrict__ part, const CalParams o, int sums_only, int it,
                                                        int may_step, double *__restrict__ ext, CalResult *__restrict__ res,
                                                        double *__restrict__ sums, int32_t *__restrict__ flag)
{
    __shared__ double sh[CAL_NS];
    __shared__ double ws[CAL_WS];
    const int job = blockIdx.x;
    if (res[job].status != CAL_RUNNING) return;
    if (threadIdx.x < CAL_NS) {
        // up to CAL_MAX_BLOCKS partials, added one after another: the loads go out sixteen at a time, the order of the additions stays
        const double *__restrict__ P = part + (int64_t)job * nb * CAL_NS + threadIdx.x;
        double a = 0.0;
        int b = 0;
        for (; b + 16 <= nb; b += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = P[(int64_t)(b + k) * CAL_NS];
#pragma unroll
            for (int k = 0; k < 16; ++k) a += v[k];
        }
        for (; b < nb; ++b) a += P[(int64_t)b * CAL_NS];
        sh[threadIdx.x] = a;
        sums[(int64_t)job * CAL_NS + threadIdx.x] = a;
    }
    __syncthreads();
    if (sums_only || threadIdx.x != 0) return;
    CalResult &r = res[job];
    double *T = ext + 12 * (int64_t)job;
    const int st = cal_step(sh, o, may_step != 0, T, T + 9, ws, r);
    r.iterations = it;                  // steps taken before this linearisation
    if (st == CAL_RUNNING) *flag = 1;
    else r.status = st;
}

int32_t check_opts(const lvba_calib_opts *opts, lvba_calib_opts &o)
{
    lvba_calib_default_opts(&o);
    if (opts) o = *opts;
    if (o.max_iterations < 1 || o.max_iterations > 1000) return lvba_fail(LVBA_ERR_ARG, "max_iterations %d (1 .. 1000)", o.max_iterations);
    if (o.min_records < 0 || !(o.max_error_px >= 0.0) || !(o.min_eig_ratio >= 0.0) || !(o.eps_rot >= 0.0) || !(o.eps_trans >= 0.0) ||
        !std::isfinite(o.max_error_px) || !std::isfinite(o.min_eig_ratio))
        return lvba_fail(LVBA_ERR_ARG, "options: min_records %lld, max_error_px %g, min_eig_ratio %g, eps_rot %g, eps_trans %g (all >= 0)",
                         (long long)o.min_records, o.max_error_px, o.min_eig_ratio, o.eps_rot, o.eps_trans);
    if (o.loss_kind < LVBA_LOSS_TRIVIAL || o.loss_kind > LVBA_LOSS_TUKEY ||
        (o.loss_kind != LVBA_LOSS_TRIVIAL && !(o.loss_scale_px > 0.0 && std::isfinite(o.loss_scale_px))))
        return lvba_fail(LVBA_ERR_ARG, "loss: kind %d, scale %g px (a known kind; finite and > 0 unless trivial)", o.loss_kind, o.loss_scale_px);
    return LVBA_OK;
}

CalParams params_of(const double *intr, const lvba_calib_opts &o)
{
    CalParams par{};
    par.fx = intr[0]; par.fy = intr[1]; par.max_error_px = o.max_error_px; par.loss_scale = o.loss_scale_px;
    par.min_eig_ratio = o.min_eig_ratio; par.eps_rot = o.eps_rot; par.eps_trans = o.eps_trans; par.min_records = o.min_records;
    par.loss_kind = o.loss_kind;
    return par;
}

// what both iterations refuse beyond null pointers and options: intrinsics, poses, initial extrinsics, the pair table, the records' runs
int32_t check_inputs(int32_t M, const double *poses, const double *intr, int32_t n_pairs, const int32_t *img_a, const int32_t *img_b, int64_t n,
                     const int32_t *pair, int32_t n_jobs, const double *Rci, const double *tci)
{
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    for (int64_t k = 0; k < 12 * (int64_t)M; ++k)
        if (!std::isfinite(poses[k])) return lvba_fail(LVBA_ERR_ARG, "body pose %lld is not finite", (long long)(k / 12));
    for (int64_t k = 0; k < (int64_t)n_jobs; ++k) {
        for (int a = 0; a < 9; ++a)
            if (!std::isfinite(Rci[9 * k + a])) return lvba_fail(LVBA_ERR_ARG, "job %lld: non-finite initial rotation", (long long)k);
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(tci[3 * k + a])) return lvba_fail(LVBA_ERR_ARG, "job %lld: non-finite initial translation", (long long)k);
    }
    for (int32_t p = 0; p < n_pairs; ++p) TRY(check_image_pair(img_a[p], img_b[p], M));
    {
        std::vector<uint8_t> seen((size_t)n_pairs, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t p = pair[i];
            if (p < 0 || p >= n_pairs) return lvba_fail(LVBA_ERR_ARG, "record %lld: pair %d of %d", (long long)i, p, n_pairs);
            if (i > 0 && p == pair[i - 1]) continue;
            if (seen[p]) return lvba_fail(LVBA_ERR_ARG, "record %lld: the records of pair %d are not in one run", (long long)i, p);
            seen[p] = 1;
        }
    }
    return LVBA_OK;
}

// Both entry points.  sums_only: one linearisation per job, H / g / cost / n_used / sum_sq out; else the iteration and every
// per-job output of lvba_calib_extrinsic.  Nothing is written before the arguments have passed.
int32_t calib_run(int32_t device, int32_t M, const double *poses, const double *intr, int32_t n_pairs, const int32_t *img_a,
                  const int32_t *img_b, int64_t n, const int32_t *pair, const float *uv, const double *Xb, int32_t n_jobs, const double *Rci,
                  const double *tci, const lvba_calib_opts *opts, bool sums_only, double *H, double *g, double *cost, int64_t *n_used,
                  double *sum_sq, double *Rci_out, double *tci_out, int32_t *status, int32_t *iterations, double *rmse_px, int32_t *n_held,
                  double *eigenvalues, double *eigenvectors)
{
    if (!poses || !intr || !Rci || !tci || !H || !cost || !n_used || M < 1 || n_pairs < 0 || n < 0 || n_jobs < 1 ||
        (n_pairs > 0 && (!img_a || !img_b)) || (n > 0 && (!pair || !uv || !Xb)) ||
        (sums_only ? !(g && sum_sq) : !(Rci_out && tci_out && status && iterations && rmse_px && n_held && eigenvalues && eigenvectors)))
        return lvba_fail(LVBA_ERR_ARG, "null argument, M < 1, n_jobs < 1 or a negative count");
    lvba_calib_opts o;
    TRY(check_opts(opts, o));
    TRY(check_inputs(M, poses, intr, n_pairs, img_a, img_b, n, pair, n_jobs, Rci, tci));
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    CalParams par{};
    par.fx = intr[0]; par.fy = intr[1]; par.max_error_px = o.max_error_px; par.loss_scale = o.loss_scale_px;
    par.min_eig_ratio = o.min_eig_ratio; par.eps_rot = o.eps_rot; par.eps_trans = o.eps_trans; par.min_records = o.min_records;
    par.loss_kind = o.loss_kind;
    const int max_steps = sums_only ? 0 : o.max_iterations;   // then one more linearisation: what is reported is of the final extrinsic
    const size_t nj = (size_t)n_jobs, np = (size_t)n_pairs, nr = (size_t)n;
    const int nb = cal_blocks(n);
    PinnedWords words;
    HIPCHK(PinnedCache::get().acquire((void **)&words.p, 4096)); // (>= 1001 words; one size for the cache's sake)
    int32_t *d_words = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&d_words, words.p, 0));
    for (int it = 0; it <= max_steps; ++it) words.p[it] = 0;
    std::vector<CalResult> hres(nj);
    std::vector<double> hext(12 * nj);
    for (size_t k = 0; k < nj; ++k) {
        hres[k] = CalResult{};
        hres[k].status = CAL_RUNNING;
        std::copy_n(Rci + 9 * k, 9, &hext[12 * k]);
        std::copy_n(tci + 3 * k, 3, &hext[12 * k + 9]);
    }
    DevArr<double> d_poses(s), d_pairT(s), d_xy(s), d_Xb(s), d_ext(s), d_part(s), d_sums(s);
    DevArr<int32_t> d_a(s), d_b(s), d_pair(s);
    DevArr<float> d_uv(s);
    DevArr<CalResult> d_res(s);
    HIPCHK(d_poses.alloc(12 * (size_t)M)); HIPCHK(d_pairT.alloc(12 * np)); HIPCHK(d_xy.alloc(2 * nr)); HIPCHK(d_Xb.alloc(3 * nr));
    HIPCHK(d_ext.alloc(12 * nj)); HIPCHK(d_part.alloc((size_t)CAL_NS * (size_t)nb * nj)); HIPCHK(d_sums.alloc((size_t)CAL_NS * nj));
    HIPCHK(d_a.alloc(np)); HIPCHK(d_b.alloc(np)); HIPCHK(d_pair.alloc(nr)); HIPCHK(d_uv.alloc(2 * nr)); HIPCHK(d_res.alloc(nj));
    HIPCHK(d_poses.upload(poses, 12 * (size_t)M));
    if (np) { HIPCHK(d_a.upload(img_a, np)); HIPCHK(d_b.upload(img_b, np)); }
    if (nr) { HIPCHK(d_pair.upload(pair, nr)); HIPCHK(d_uv.upload(uv, 2 * nr)); HIPCHK(d_Xb.upload(Xb, 3 * nr)); }
    HIPCHK(d_ext.upload(hext.data(), 12 * nj));
    HIPCHK(d_res.upload(hres.data(), nj));
    HIPCHK(d_sums.zero_async((size_t)CAL_NS * nj));
    if (std::max<int64_t>(n, n_pairs) > 0) {
        calib_prepare_kernel<<<grid_for(std::max<int64_t>(n, n_pairs), 256), 256, 0, s>>>(n, n_pairs, d_poses, d_a, d_b, d_uv, d_Xb,
                                                                                        trk_intr_of(intr), d_pairT, d_xy);
        HIPCHK(hipGetLastError());
    }
    for (int it = 0; it <= max_steps; ++it) {
        calib_linearize_kernel<<<dim3((unsigned)nb, (unsigned)n_jobs), CAL_BLOCK, 0, s>>>(n, d_pair, d_xy, d_Xb, d_pairT, d_ext, d_res, par,
                                                                                         d_part);
        HIPCHK(hipGetLastError());
        calib_step_kernel<<<(unsigned)n_jobs, 64, 0, s>>>(nb, d_part, par, sums_only ? 1 : 0, it, it < max_steps ? 1 : 0, d_ext, d_res, d_sums,
                                                          d_words + it);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        if (!words.p[it]) break; // every job has finished
    }
    std::vector<double> hsums((size_t)CAL_NS * nj);
    HIPCHK(d_sums.download(hsums.data(), hsums.size()));
    if (!sums_only) {
        HIPCHK(d_ext.download(hext.data(), 12 * nj));
        HIPCHK(d_res.download(hres.data(), nj));
    }
    for (size_t k = 0; k < nj; ++k) {
        const double *sk = hsums.data() + (size_t)CAL_NS * k;
        cal_expand(sk, H + 36 * k);
        cost[k] = sk[CAL_COST];
        n_used[k] = (int64_t)sk[CAL_CNT];
        if (sums_only) {
            for (int a = 0; a < 6; ++a) g[6 * k + a] = sk[CAL_G0 + a];
            sum_sq[k] = sk[CAL_SSQ];
            continue;
        }
        const CalResult &r = hres[k];
        std::copy_n(&hext[12 * k], 9, Rci_out + 9 * k);
        std::copy_n(&hext[12 * k + 9], 3, tci_out + 3 * k);
        status[k] = r.status; iterations[k] = r.iterations; rmse_px[k] = r.rmse; n_held[k] = r.n_held;
        std::copy_n(r.eig, 6, eigenvalues + 6 * k);
        std::copy_n(r.vec, 36, eigenvectors + 36 * k);
    }
    return LVBA_OK;
}

// ---- the time offset as a seventh parameter (lvba_calib_*_td; calib_td_device.h, DESIGN.md §10o "time offset").  The skeleton above
// with one more small launch per iteration: the pair table depends on every job's current td, so calib_td_pairs_kernel rewrites it
// before each linearisation; calib_prepare_kernel (with no pairs) still undistorts the targets once per call.

// ext [jobs][CAL_TD_EXT]; pairE [jobs][n_pairs][CAL_TD_ROW]: a thread per (job, pair)
__global__ __launch_bounds__(256) void calib_td_pairs_kernel(int32_t n_pairs, const double *__restrict__ poses, const double *__restrict__ twists,
                                                             const int32_t *__restrict__ img_a, const int32_t *__restrict__ img_b,
                                                             const double *__restrict__ ext, const CalTdResult *__restrict__ res,
                                                             double *__restrict__ pairE)
{
    const int job = blockIdx.y;
    if (res[job].status != CAL_RUNNING) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const int64_t a = img_a[i], b = img_b[i];
    double E[CAL_TD_ROW];
    cal_td_pair(poses + 12 * a, poses + 12 * b, twists + 6 * a, twists + 6 * b, ext[CAL_TD_EXT * (int64_t)job + 12], E);
    double *__restrict__ out = pairE + CAL_TD_ROW * ((int64_t)job * n_pairs + i);
#pragma unroll
    for (int k = 0; k < CAL_TD_ROW; ++k) out[k] = E[k];
}

// calib_linearize_kernel's partition and reduction at CAL_TD_NS sums; part [jobs][gridDim.x][CAL_TD_NS]
__global__ __launch_bounds__(CAL_BLOCK) void calib_td_linearize_kernel(int64_t n, int32_t n_pairs, const int32_t *__restrict__ pair,
                                                                       const double *__restrict__ xy, const double *__restrict__ Xb,
                                                                       const double *__restrict__ pairE, const double *__restrict__ ext,
                                                                       const CalTdResult *__restrict__ res, const CalParams o,
                                                                       double *__restrict__ part)
{
    __shared__ double red[CAL_BLOCK / 64][CAL_TD_NS];
    const int job = blockIdx.y;
    if (res[job].status != CAL_RUNNING) return;
    const int nb = cal_blocks(n);
    if ((int)blockIdx.x >= nb) return;
    double T[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) T[a] = ext[CAL_TD_EXT * (int64_t)job + a];
    const double *__restrict__ table = pairE + (int64_t)CAL_TD_ROW * n_pairs * job;
    double s[CAL_TD_NS];
#pragma unroll
    for (int q = 0; q < CAL_TD_NS; ++q) s[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * CAL_BLOCK + threadIdx.x; i < n; i += (int64_t)nb * CAL_BLOCK) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        if (!(x == x && y == y)) continue;
        const double X[3] = {Xb[3 * i], Xb[3 * i + 1], Xb[3 * i + 2]};
        const double *__restrict__ Ep = table + CAL_TD_ROW * (int64_t)pair[i];
        double E[CAL_TD_ROW];
#pragma unroll
        for (int a = 0; a < CAL_TD_ROW; ++a) E[a] = Ep[a];
        cal_td_record(T, T + 9, E, x, y, X, o, s);
    }
#pragma unroll
    for (int q = 0; q < CAL_TD_NS; ++q) s[q] = wave_sum_to_lane63(s[q]); // (a lane without a source adds 0.0)
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < CAL_TD_NS; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < CAL_TD_NS) {
        const int q = threadIdx.x;
        part[((int64_t)job * gridDim.x + blockIdx.x) * CAL_TD_NS + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// calib_step_kernel at seven parameters: lanes 0 .. 38 add the partials, lane 0 takes cal_td_step
__global__ __launch_bounds__(64) void calib_td_step_kernel(int nb, const double *__restrict__ part, const CalTdParams o, int sums_only, int it,
                                                           int may_step, double *__restrict__ ext, CalTdResult *__restrict__ res,
                                                           double *__restrict__ sums, int32_t *__restrict__ flag)
{
    __shared__ double sh[CAL_TD_NS];
    __shared__ double ws[CAL_TD_WS];
    const int job = blockIdx.x;
    if (res[job].status != CAL_RUNNING) return;
    if (threadIdx.x < CAL_TD_NS) {
        // as calib_step_kernel: the loads go out sixteen at a time, the order of the additions stays
        const double *__restrict__ P = part + (int64_t)job * nb * CAL_TD_NS + threadIdx.x;
        double a = 0.0;
        int b = 0;
        for (; b + 16 <= nb; b += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = P[(int64_t)(b + k) * CAL_TD_NS];
#pragma unroll
            for (int k = 0; k < 16; ++k) a += v[k];
        }
        for (; b < nb; ++b) a += P[(int64_t)b * CAL_TD_NS];
        sh[threadIdx.x] = a;
        sums[(int64_t)job * CAL_TD_NS + threadIdx.x] = a;
    }
    __syncthreads();
    if (sums_only || threadIdx.x != 0) return;
    CalTdResult &r = res[job];
    const int st = cal_td_step(sh, o, may_step != 0, ext + CAL_TD_EXT * (int64_t)job, ws, r);
    r.iterations = it;                  // steps taken before this linearisation
    if (st == CAL_RUNNING) *flag = 1;
    else r.status = st;
}

int32_t check_td_opts(const lvba_calib_td_opts *opts, lvba_calib_td_opts &o)
{
    lvba_calib_td_default_opts(&o);
    if (opts) o = *opts;
    lvba_calib_opts base;
    TRY(check_opts(&o.calib, base));
    if (!(o.eps_td_s >= 0.0) || !(o.max_abs_td_s > 0.0))
        return lvba_fail(LVBA_ERR_ARG, "options: eps_td_s %g (>= 0), max_abs_td_s %g (> 0)", o.eps_td_s, o.max_abs_td_s);
    return LVBA_OK;
}

// Both td entry points, as calib_run.  Outputs per job: H [49] (information), g [7], eigenvalues [7], eigenvectors [49].
int32_t calib_td_run(int32_t device, int32_t M, const double *poses, const double *twists, const double *intr, int32_t n_pairs,
                     const int32_t *img_a, const int32_t *img_b, int64_t n, const int32_t *pair, const float *uv, const double *Xb,
                     int32_t n_jobs, const double *Rci, const double *tci, const double *td0, const lvba_calib_td_opts *opts, bool sums_only,
                     double *H, double *g, double *cost, int64_t *n_used, double *sum_sq, double *Rci_out, double *tci_out, double *td_out,
                     int32_t *status, int32_t *iterations, double *rmse_px, int32_t *n_held, double *eigenvalues, double *eigenvectors)
{
    if (!poses || !twists || !intr || !Rci || !tci || !td0 || !H || !cost || !n_used || M < 1 || n_pairs < 0 || n < 0 || n_jobs < 1 ||
        (n_pairs > 0 && (!img_a || !img_b)) || (n > 0 && (!pair || !uv || !Xb)) ||
        (sums_only ? !(g && sum_sq)
                   : !(Rci_out && tci_out && td_out && status && iterations && rmse_px && n_held && eigenvalues && eigenvectors)))
        return lvba_fail(LVBA_ERR_ARG, "null argument, M < 1, n_jobs < 1 or a negative count");
    lvba_calib_td_opts o;
    TRY(check_td_opts(opts, o));
    TRY(check_inputs(M, poses, intr, n_pairs, img_a, img_b, n, pair, n_jobs, Rci, tci));
    for (int64_t k = 0; k < 6 * (int64_t)M; ++k)
        if (!std::isfinite(twists[k])) return lvba_fail(LVBA_ERR_ARG, "body twist %lld is not finite", (long long)(k / 6));
    for (int32_t k = 0; k < n_jobs; ++k)
        if (!std::isfinite(td0[k]) || std::fabs(td0[k]) > o.max_abs_td_s)
            return lvba_fail(LVBA_ERR_ARG, "job %d: initial time offset %g s (finite, at most max_abs_td_s = %g)", k, td0[k], o.max_abs_td_s);
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    CalTdParams par{};
    par.cal = params_of(intr, o.calib);
    par.eps_td = o.eps_td_s; par.max_abs_td = o.max_abs_td_s;
    const int max_steps = sums_only ? 0 : o.calib.max_iterations;
    const size_t nj = (size_t)n_jobs, np = (size_t)n_pairs, nr = (size_t)n;
    const int nb = cal_blocks(n);
    PinnedWords words;
    HIPCHK(PinnedCache::get().acquire((void **)&words.p, 4096));
    int32_t *d_words = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&d_words, words.p, 0));
    for (int it = 0; it <= max_steps; ++it) words.p[it] = 0;
    std::vector<CalTdResult> hres(nj);
    std::vector<double> hext(CAL_TD_EXT * nj);
    for (size_t k = 0; k < nj; ++k) {
        hres[k] = CalTdResult{};
        hres[k].status = CAL_RUNNING;
        std::copy_n(Rci + 9 * k, 9, &hext[CAL_TD_EXT * k]);
        std::copy_n(tci + 3 * k, 3, &hext[CAL_TD_EXT * k + 9]);
        hext[CAL_TD_EXT * k + 12] = td0[k];
    }
    DevArr<double> d_poses(s), d_twists(s), d_pairE(s), d_xy(s), d_Xb(s), d_ext(s), d_part(s), d_sums(s);
    DevArr<int32_t> d_a(s), d_b(s), d_pair(s);
    DevArr<float> d_uv(s);
    DevArr<CalTdResult> d_res(s);
    HIPCHK(d_poses.alloc(12 * (size_t)M)); HIPCHK(d_twists.alloc(6 * (size_t)M)); HIPCHK(d_pairE.alloc((size_t)CAL_TD_ROW * np * nj));
    HIPCHK(d_xy.alloc(2 * nr)); HIPCHK(d_Xb.alloc(3 * nr)); HIPCHK(d_ext.alloc(CAL_TD_EXT * nj));
    HIPCHK(d_part.alloc((size_t)CAL_TD_NS * (size_t)nb * nj)); HIPCHK(d_sums.alloc((size_t)CAL_TD_NS * nj));
    HIPCHK(d_a.alloc(np)); HIPCHK(d_b.alloc(np)); HIPCHK(d_pair.alloc(nr)); HIPCHK(d_uv.alloc(2 * nr)); HIPCHK(d_res.alloc(nj));
    HIPCHK(d_poses.upload(poses, 12 * (size_t)M));
    HIPCHK(d_twists.upload(twists, 6 * (size_t)M));
    if (np) { HIPCHK(d_a.upload(img_a, np)); HIPCHK(d_b.upload(img_b, np)); }
    if (nr) { HIPCHK(d_pair.upload(pair, nr)); HIPCHK(d_uv.upload(uv, 2 * nr)); HIPCHK(d_Xb.upload(Xb, 3 * nr)); }
    HIPCHK(d_ext.upload(hext.data(), CAL_TD_EXT * nj));
    HIPCHK(d_res.upload(hres.data(), nj));
    HIPCHK(d_sums.zero_async((size_t)CAL_TD_NS * nj));
    if (n > 0) {
        calib_prepare_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, 0, d_poses, d_a, d_b, d_uv, d_Xb, trk_intr_of(intr), nullptr, d_xy);
        HIPCHK(hipGetLastError());
    }
    for (int it = 0; it <= max_steps; ++it) {
        if (n_pairs > 0) {
            calib_td_pairs_kernel<<<dim3(grid_for(n_pairs, 256), (unsigned)n_jobs), 256, 0, s>>>(n_pairs, d_poses, d_twists, d_a, d_b, d_ext,
                                                                                               d_res, d_pairE);
            HIPCHK(hipGetLastError());
        }
        calib_td_linearize_kernel<<<dim3((unsigned)nb, (unsigned)n_jobs), CAL_BLOCK, 0, s>>>(n, n_pairs, d_pair, d_xy, d_Xb, d_pairE, d_ext,
                                                                                            d_res, par.cal, d_part);
        HIPCHK(hipGetLastError());
        calib_td_step_kernel<<<(unsigned)n_jobs, 64, 0, s>>>(nb, d_part, par, sums_only ? 1 : 0, it, it < max_steps ? 1 : 0, d_ext, d_res,
                                                             d_sums, d_words + it);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        if (!words.p[it]) break; // every job has finished
    }
    std::vector<double> hsums((size_t)CAL_TD_NS * nj);
    HIPCHK(d_sums.download(hsums.data(), hsums.size()));
    if (!sums_only) {
        HIPCHK(d_ext.download(hext.data(), CAL_TD_EXT * nj));
        HIPCHK(d_res.download(hres.data(), nj));
    }
    for (size_t k = 0; k < nj; ++k) {
        const double *sk = hsums.data() + (size_t)CAL_TD_NS * k;
        cal_expand_n(sk, H + 49 * k, CAL_TD_N);
        cost[k] = sk[CAL_TD_COST];
        n_used[k] = (int64_t)sk[CAL_TD_CNT];
        if (sums_only) {
            for (int a = 0; a < CAL_TD_N; ++a) g[CAL_TD_N * k + a] = sk[CAL_TD_G0 + a];
            sum_sq[k] = sk[CAL_TD_SSQ];
            continue;
        }
        const CalTdResult &r = hres[k];
        const bool out_of_range = r.status == CAL_TD_OUT_OF_RANGE;   // the job's start values come back bit for bit
        std::copy_n(out_of_range ? Rci + 9 * k : &hext[CAL_TD_EXT * k], 9, Rci_out + 9 * k);
        std::copy_n(out_of_range ? tci + 3 * k : &hext[CAL_TD_EXT * k + 9], 3, tci_out + 3 * k);
        td_out[k] = out_of_range ? td0[k] : hext[CAL_TD_EXT * k + 12];
        status[k] = r.status; iterations[k] = r.iterations; rmse_px[k] = r.rmse; n_held[k] = r.n_held;
        std::copy_n(r.eig, CAL_TD_N, eigenvalues + CAL_TD_N * k);
        std::copy_n(r.vec, 49, eigenvectors + 49 * k);
    }
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_calib_default_opts(lvba_calib_opts *o)
{
    if (!o) return;
    *o = lvba_calib_opts{};
    o->max_iterations = 20;
    o->loss_kind = LVBA_LOSS_HUBER;
    o->min_records = 100;
    o->loss_scale_px = 2.0;     // the prototype's value, not tuned on data
    o->max_error_px = 0.0;      // no gate
    o->min_eig_ratio = 1e-6;    // between the prototype's two regimes, not measured on recorded data
    o->eps_rot = 1e-10;
    o->eps_trans = 1e-10;
}

extern "C" int32_t lvba_calib_linearize(int32_t device, int32_t n_images, const double *body_poses, const double *intr, int32_t n_pairs,
                                        const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair, const float *uv_a,
                                        const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const lvba_calib_opts *opts,
                                        double *H, double *g, double *cost, int64_t *n_used, double *sum_sq)
{
    return calib_run(device, n_images, body_poses, intr, n_pairs, img_a, img_b, n_records, pair, uv_a, Xb, n_jobs, Rci, tci, opts, true, H, g,
                     cost, n_used, sum_sq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int32_t lvba_calib_extrinsic(int32_t device, int32_t n_images, const double *body_poses, const double *intr, int32_t n_pairs,
                                        const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair, const float *uv_a,
                                        const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const lvba_calib_opts *opts,
                                        double *Rci_out, double *tci_out, int32_t *status, int32_t *iterations, int64_t *n_used,
                                        double *rmse_px, double *cost, int32_t *n_held, double *eigenvalues, double *eigenvectors,
                                        double *information)
{
    return calib_run(device, n_images, body_poses, intr, n_pairs, img_a, img_b, n_records, pair, uv_a, Xb, n_jobs, Rci, tci, opts, false,
                     information, nullptr, cost, n_used, nullptr, Rci_out, tci_out, status, iterations, rmse_px, n_held, eigenvalues,
                     eigenvectors);
}

extern "C" void lvba_calib_td_default_opts(lvba_calib_td_opts *o)
{
    if (!o) return;
    *o = lvba_calib_td_opts{};
    lvba_calib_default_opts(&o->calib);
    o->eps_td_s = 1e-10;        // eps_rot's reasoning: far below what the data resolve, far above the step's rounding
    o->max_abs_td_s = 0.2;      // beyond it a constant twist is no description of the motion; not tuned on data
}

extern "C" int32_t lvba_calib_linearize_td(int32_t device, int32_t n_images, const double *body_poses, const double *body_twists,
                                           const double *intr, int32_t n_pairs, const int32_t *img_a, const int32_t *img_b, int64_t n_records,
                                           const int32_t *pair, const float *uv_a, const double *Xb, int32_t n_jobs, const double *Rci,
                                           const double *tci, const double *td0, const lvba_calib_td_opts *opts, double *H, double *g,
                                           double *cost, int64_t *n_used, double *sum_sq)
{
    return calib_td_run(device, n_images, body_poses, body_twists, intr, n_pairs, img_a, img_b, n_records, pair, uv_a, Xb, n_jobs, Rci, tci,
                        td0, opts, true, H, g, cost, n_used, sum_sq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr);
}

extern "C" int32_t lvba_calib_extrinsic_td(int32_t device, int32_t n_images, const double *body_poses, const double *body_twists,
                                           const double *intr, int32_t n_pairs, const int32_t *img_a, const int32_t *img_b, int64_t n_records,
                                           const int32_t *pair, const float *uv_a, const double *Xb, int32_t n_jobs, const double *Rci,
                                           const double *tci, const double *td0, const lvba_calib_td_opts *opts, double *Rci_out,
                                           double *tci_out, double *td_out, int32_t *status, int32_t *iterations, int64_t *n_used,
                                           double *rmse_px, double *cost, int32_t *n_held, double *eigenvalues, double *eigenvectors,
                                           double *information)
{
    return calib_td_run(device, n_images, body_poses, body_twists, intr, n_pairs, img_a, img_b, n_records, pair, uv_a, Xb, n_jobs, Rci, tci,
                        td0, opts, false, information, nullptr, cost, n_used, nullptr, Rci_out, tci_out, td_out, status, iterations, rmse_px,
                        n_held, eigenvalues, eigenvectors);
}
