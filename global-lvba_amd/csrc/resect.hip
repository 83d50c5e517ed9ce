// resect.hip -- camera resectioning: P3P RANSAC over the 2-D to 3-D correspondences of many images at once (lvba_resect_*; the rule
// is in include/lvba_hip.h, its scalar pieces in resect_device.h).
//
// What is this stage's own, on the skeleton of ransac_batch.h (DESIGN.md §10k says which piece is whose; §10n why 40-byte records):
//   (image_set.hip)           the pixels undistorted once per call: an ImageSet whose "images" are the jobs.
//   resect_pack_kernel        a thread per correspondence: its record (x, y, X) of RESECT_REC = 5 doubles, an unusable one marked by NaN.
//   resect_hypothesis_kernel  a lane draws its four positions, reads those records from global memory and solves in registers (the
//                             solver's 3 x 3 matrices are indexed by compile-time constants only, its choices are select chains: no
//                             scratch memory).  The pose stays in twelve register pairs; the job's records are staged in LDS in
//                             chunks of RESECT_CHUNK, which every lane walks (a broadcast read).
//   resect_refine_kernel      a workgroup per job: per Gauss-Newton step the 27 sums over the inliers (per-thread strides, then
//                             wave_ops.h' fixed trees), the 6 x 6 solve in one lane (constant trip counts: the matrix stays in
//                             registers), after a round the rescore; then status, rmse and information at the final pose.
//   ResectInlier, ResectEmit  the inlier test of the mask kernel; an inlier is written as its position within its job.
//   resect_lift_kernel        a thread per keypoint: match_device.h' match_lift through the image's depth image.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "segments.h"
#include "image_set.h"
#include "match_device.h"
#include "resect_device.h"
#include "ransac_batch.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int RESECT_CHUNK = 1024;          // correspondences staged in LDS at a time, 40 bytes each
constexpr int REFINE_BLOCK = 256;

struct ResectTask {
    RansacSpan span;                // the job's correspondences in the call's list, its block records
    int32_t id;
};
typedef RansacBest<12> ResectBest;  // the model is the pose: R [9], then t [3]

// rec [n][RESECT_REC]
__global__ __launch_bounds__(256) void resect_pack_kernel(int64_t n, const double *__restrict__ xy, const double *__restrict__ world,
                                                          double *__restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double X[3] = {world[3 * i], world[3 * i + 1], world[3 * i + 2]};
    double r[RESECT_REC];
    resect_pack(xy[2 * i], xy[2 * i + 1], X, r);
#pragma unroll
    for (int k = 0; k < RESECT_REC; ++k) rec[RESECT_REC * i + k] = r[k];
}

// tiles [n_tiles]; blk, diag_pose, diag_count: see ransac_block_best
__global__ __launch_bounds__(RANSAC_HB) void resect_hypothesis_kernel(const ResectTask *__restrict__ tasks, const RansacTile *__restrict__ tiles,
                                                                      const double *__restrict__ rec, uint64_t seed, int H, double fx,
                                                                      double fy, double rho, ResectBest *__restrict__ blk,
                                                                      double *__restrict__ diag_pose, int32_t *__restrict__ diag_count)
{
    __shared__ double lds[RESECT_REC * RESECT_CHUNK];
    const RansacLane ln = ransac_lane(tiles, H);
    const ResectTask &task = tasks[ln.task];
    const int lane = threadIdx.x, m = task.span.m;
    const double *__restrict__ jr = rec + RESECT_REC * task.span.off;
    double P[12] = {};              // R, then t
    double *const R = P, *const t = P + 9;
    bool valid = false;
    if (ln.live) {
        int32_t idx[RESECT_K];
        ransac_sample<RESECT_K>(ransac_key(seed, task.id, -1, ln.h), m, idx);
        double c[RESECT_K][RESECT_REC];
#pragma unroll
        for (int j = 0; j < RESECT_K; ++j)
#pragma unroll
            for (int k = 0; k < RESECT_REC; ++k) c[j][k] = jr[RESECT_REC * (int64_t)idx[j] + k];
        valid = resect_p3p(c[0], c[1], c[2], c[3], fx, fy, R, t);
    }
    int32_t count = 0;
    for (int c0 = 0; c0 < m; c0 += RESECT_CHUNK) {
        const int n = min(RESECT_CHUNK, m - c0);
        for (int i = lane; i < RESECT_REC * n; i += RANSAC_HB) lds[i] = jr[RESECT_REC * (int64_t)c0 + i];
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const double *p = lds + RESECT_REC * i;
            count += resect_inlier(R, t, fx, fy, rho, p[0], p[1], p[2], p[3], p[4]) ? 1 : 0;
        }
        __syncthreads();
    }
    if (!valid) count = -1;
    ransac_block_best<12>(ln, count, P, blk, diag_pose, diag_count);
}

// the number of inliers of (R, t) among the job's records, in every thread
__device__ __forceinline__ int32_t block_count(const double *__restrict__ jr, int m, const double *R, const double *t, double fx, double fy,
                                               double rho, double *red)
{
    int32_t c = 0;
    for (int i = threadIdx.x; i < m; i += REFINE_BLOCK) {
        const double *p = jr + RESECT_REC * (int64_t)i;
        c += resect_inlier(R, t, fx, fy, rho, p[0], p[1], p[2], p[3], p[4]) ? 1 : 0;
    }
    return (int32_t)block_sum_all<REFINE_BLOCK / 64>((double)c, red); // integers below 2^31: exact in fp64 in any order
}
// sT [n_sums] = the sums of resect_accumulate at (P, q) over the inliers of (R, t)
__device__ __forceinline__ void block_sums(const double *__restrict__ jr, int m, const double *R, const double *t, const double *P,
                                           const double *q, double fx, double fy, double rho, double *red, double *sT)
{
    double acc[RESECT_NSUM];
#pragma unroll
    for (int k = 0; k < RESECT_NSUM; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < m; i += REFINE_BLOCK) {
        const double *p = jr + RESECT_REC * (int64_t)i;
        if (resect_inlier(R, t, fx, fy, rho, p[0], p[1], p[2], p[3], p[4])) resect_accumulate(P, q, fx, fy, p[0], p[1], p[2], p[3], p[4], acc);
    }
#pragma unroll
    for (int k = 0; k < RESECT_NSUM; ++k) {
        const double sum = block_sum_all<REFINE_BLOCK / 64>(acc[k], red);
        if (threadIdx.x == 0) sT[k] = sum;
    }
}

// R_out [J][9], t_out [J][3], status, n_inliers, best_h, rmse [J], info [J][36]: the job's result after `rounds` refinement rounds
__global__ __launch_bounds__(REFINE_BLOCK) void resect_refine_kernel(const ResectTask *__restrict__ tasks, const double *__restrict__ rec,
                                                                     double fx, double fy, double rho, int rounds, int min_inliers,
                                                                     const ResectBest *__restrict__ res, double *__restrict__ R_out,
                                                                     double *__restrict__ t_out, int32_t *__restrict__ status,
                                                                     int32_t *__restrict__ n_inliers, int32_t *__restrict__ best_h,
                                                                     double *__restrict__ rmse, double *__restrict__ info)
{
    __shared__ double red[REFINE_BLOCK / 64];
    __shared__ double sT[RESECT_NSUM], sP[12];
    __shared__ int s_ok;
    const int j = blockIdx.x, tid = threadIdx.x;
    const ResectTask &task = tasks[j];
    const int m = task.span.m;
    const double *__restrict__ jr = rec + RESECT_REC * task.span.off;
    const ResectBest b = res[j];
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = b.model[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = b.model[9 + k];
    int32_t count = b.count;
    for (int round = 0; round < rounds && count > 0; ++round) { // every condition below is the same in all threads
        double P[9], q[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = t[k];
        bool ok = true;
        for (int step = 0; step < RESECT_GN_STEPS && ok; ++step) {
            block_sums(jr, m, R, t, P, q, fx, fy, rho, red, sT);
            if (tid == 0) {
                double Pn[9], qn[3], N36[36];
#pragma unroll
                for (int k = 0; k < 9; ++k) Pn[k] = P[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) qn[k] = q[k];
                s_ok = resect_step(sT, N36, Pn, qn) ? 1 : 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) sP[k] = Pn[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) sP[9 + k] = qn[k];
            }
            __syncthreads();
            ok = s_ok != 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) P[k] = sP[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = sP[9 + k];
            __syncthreads(); // sP and s_ok are free again
        }
        if (!ok) break;
        const int32_t cn = block_count(jr, m, P, q, fx, fy, rho, red);
        if (cn < count) break;                                            // kept iff not smaller
        count = cn;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = P[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = q[k];
    }
    if (count > 0) block_sums(jr, m, R, t, R, t, fx, fy, rho, red, sT);
    if (tid != 0) return;
    status[j] = ransac_status(m, RESECT_K, min_inliers, count);
    n_inliers[j] = count > 0 ? count : 0;
    best_h[j] = b.h;
#pragma unroll
    for (int k = 0; k < 9; ++k) R_out[9 * (int64_t)j + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t_out[3 * (int64_t)j + k] = t[k];
    double *I = info + 36 * (int64_t)j;
    int k = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) {
            const double v = count > 0 ? sT[k] : 0.0;
            I[6 * r + c] = v; I[6 * c + r] = v;
            ++k;
        }
    rmse[j] = count > 0 ? sqrt(sT[27] / (double)count) : 0.0;
}

// correspondence i of the call, of job j, is an inlier of the pose (R [j], t [j])
struct ResectInlier {
    const double *rec, *R, *t;
    double fx, fy, rho;
    __device__ bool operator()(const ResectTask &, int j, int64_t i) const
    {
        const double *p = rec + RESECT_REC * i;
        return resect_inlier(R + 9 * (int64_t)j, t + 3 * (int64_t)j, fx, fy, rho, p[0], p[1], p[2], p[3], p[4]);
    }
};
// an inlier is its position within its job
struct ResectEmit {
    static constexpr int WIDTH = 1;
    const ResectTask *tasks;
    int n_tasks;
    __device__ void operator()(int32_t *out, int64_t pos, int64_t i) const
    {
        const ResectTask *tk = tasks;
        out[pos] = (int32_t)(i - tk[segment_of([=](int k) { return tk[k].span.off; }, n_tasks, i)].span.off);
    }
};

// world [n][3]; img_off [n_images + 1]
__global__ __launch_bounds__(256) void resect_lift_kernel(int64_t n, int n_images, const int64_t *__restrict__ img_off,
                                                          const float *__restrict__ uv, const double *__restrict__ xy,
                                                          const float *__restrict__ depth, int width, int height,
                                                          const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                          double *__restrict__ world)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int im = segment_of(img_off, n_images, i);
    match_lift(depth + (int64_t)im * width * height, width, height, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1], Rcw + 9 * (int64_t)im,
               tcw + 3 * (int64_t)im, world + 3 * i);
}

int32_t check_opts(const lvba_resect_opts *opts, lvba_resect_opts &o)
{
    lvba_resect_default_opts(&o);
    if (opts) o = *opts;
    if (o.hypotheses < 1) return lvba_fail(LVBA_ERR_ARG, "hypotheses %d (>= 1)", o.hypotheses);
    if (o.refine_rounds < 0 || o.min_inliers < 0 || !(std::isfinite(o.max_error_px) && o.max_error_px > 0.0))
        return lvba_fail(LVBA_ERR_ARG, "options: refine_rounds %d (>= 0), min_inliers %d (>= 0), max_error_px %g (finite, > 0)", o.refine_rounds,
                         o.min_inliers, o.max_error_px);
    return LVBA_OK;
}

int32_t check_camera(const double *intr)
{
    TRY(check_intrinsics_finite(intr));
    return check_focal_lengths(intr);
}

// The records of the call's correspondences on the device: the pixels undistorted (image_set.hip), then packed with the world points.
struct Records {
    ImageSet set;
    DevArr<double> rec;
    explicit Records(hipStream_t s) : rec(s) {}
    ~Records() { image_set_free(set); }
};
int32_t make_records(hipStream_t s, int device, int32_t n_jobs, const int64_t *corr_off, const float *uv, const double *world, const double *intr,
                     Records &r)
{
    r.set = ImageSet{device, n_jobs, std::vector<int64_t>(corr_off, corr_off + n_jobs + 1)};
    const int64_t total = corr_off[n_jobs];
    HIPCHK(r.rec.alloc((size_t)RESECT_REC * (size_t)total));
    if (total == 0) return LVBA_OK;
    TRY(image_set_undistort(r.set, trk_intr_of(intr), uv, false));
    DevArr<double> d_w(s);
    HIPCHK(d_w.alloc(3 * (size_t)total)); HIPCHK(d_w.upload(world, 3 * (size_t)total));
    resect_pack_kernel<<<grid_for(total, 256), 256, 0, s>>>(total, r.set.d_xy, d_w, r.rec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s)); // the world points go with this scope
    return LVBA_OK;
}

// The hypotheses of every job with enough correspondences (ransac_run_hypotheses).  diag_pose [H][12], diag_count: null, or the
// diagnostic call's outputs.
int32_t run_hypotheses(hipStream_t s, std::vector<ResectTask> &tasks, const lvba_resect_opts &o, const double *intr, const double *d_rec,
                       DevArr<ResectTask> &d_tasks, DevArr<ResectBest> &d_blk, double *diag_pose, int32_t *diag_count)
{
    return ransac_run_hypotheses<12>(s, tasks, o.hypotheses, diag_pose ? RESECT_K : std::max(RESECT_K, o.min_inliers), d_tasks, d_blk,
                                     [&](unsigned grid, const RansacTile *tiles) {
        resect_hypothesis_kernel<<<grid, RANSAC_HB, 0, s>>>(d_tasks, tiles, d_rec, o.seed, o.hypotheses, intr[0], intr[1],
                                                            o.max_error_px, d_blk, diag_pose, diag_count);
    });
}

} // namespace

extern "C" void lvba_resect_default_opts(lvba_resect_opts *o)
{
    if (!o) return;
    *o = lvba_resect_opts{};
    o->hypotheses = 1024; o->refine_rounds = 2; o->min_inliers = 30; o->max_error_px = 8.0; o->seed = 0;
}

extern "C" int32_t lvba_resect_images(int32_t device, int32_t n_jobs, const int32_t *ids, const int64_t *corr_off, const float *uv,
                                      const double *world, const double *intr, const lvba_resect_opts *opts, int64_t capacity,
                                      int64_t *inlier_off, int32_t *inliers, double *Rcw, double *tcw, int32_t *status, int32_t *n_inliers,
                                      int32_t *best_h, double *rmse_px, double *information)
{
    if (!corr_off || !intr || !inlier_off || n_jobs < 0 || capacity < 0 ||
        (n_jobs > 0 && (!ids || !Rcw || !tcw || !status || !n_inliers || !best_h || !rmse_px || !information)) || (capacity > 0 && !inliers))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_jobs < 0 or capacity < 0");
    lvba_resect_opts o;
    TRY(check_opts(opts, o));
    TRY(check_camera(intr));
    if (n_jobs >= INT32_MAX / 2) return lvba_fail(LVBA_ERR_UNSUPPORTED, "%d jobs in one call", n_jobs);
    TRY(check_offsets("corr_off", "job", n_jobs, corr_off, INT32_MAX - 1));
    const int64_t total = corr_off[n_jobs];
    if (total >= RANSAC_MAX_ELEMENTS) return lvba_fail(LVBA_ERR_UNSUPPORTED, "%lld correspondences in one call (below 2^31)", (long long)total);
    if (total > 0 && (!uv || !world)) return lvba_fail(LVBA_ERR_ARG, "null correspondences");
    {
        std::vector<int32_t> seen(ids, ids + n_jobs);
        std::sort(seen.begin(), seen.end());
        if (n_jobs > 0 && seen[0] < 0) return lvba_fail(LVBA_ERR_ARG, "job id %d (>= 0)", seen[0]);
        for (int32_t k = 1; k < n_jobs; ++k)
            if (seen[k] == seen[k - 1]) return lvba_fail(LVBA_ERR_ARG, "job id %d is given twice", seen[k]);
    }
    TRY(check_device(device));
    std::vector<ResectTask> tasks((size_t)n_jobs);
    for (int32_t j = 0; j < n_jobs; ++j) {
        tasks[j] = ResectTask{};
        tasks[j].span.off = corr_off[j]; tasks[j].span.m = (int32_t)(corr_off[j + 1] - corr_off[j]); tasks[j].id = ids[j];
    }
    if (n_jobs == 0) { inlier_off[0] = 0; return LVBA_OK; }
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    hipStream_t s = sg.s;
    const int nj = n_jobs;
    Records recs(s);
    TRY(make_records(s, device, n_jobs, corr_off, uv, world, intr, recs));
    const double *d_rec = recs.rec;
    DevArr<ResectTask> d_tasks(s); DevArr<ResectBest> d_blk(s), d_res(s); DevArr<double> d_pose(s); DevArr<int32_t> d_int(s);
    DevArr<double> d_real(s);
    TRY(run_hypotheses(s, tasks, o, intr, d_rec, d_tasks, d_blk, nullptr, nullptr));
    HIPCHK(d_res.alloc((size_t)nj)); HIPCHK(d_pose.alloc(12 * (size_t)nj)); HIPCHK(d_int.alloc(3 * (size_t)nj));
    HIPCHK(d_real.alloc(37 * (size_t)nj));
    double *d_R = d_pose, *d_t = d_R + 9 * (size_t)nj;
    double *d_info = d_real, *d_rmse = d_info + 36 * (size_t)nj;
    int32_t *d_status = d_int, *d_cnt = d_status + nj, *d_h = d_cnt + nj;
    ransac_pick_kernel<12, ResectTask><<<grid_for(nj, 256), 256, 0, s>>>(nj, d_tasks, d_blk, d_res);
    HIPCHK(hipGetLastError());
    resect_refine_kernel<<<(unsigned)nj, REFINE_BLOCK, 0, s>>>(d_tasks, d_rec, intr[0], intr[1], o.max_error_px, o.refine_rounds,
                                                              o.min_inliers, d_res, d_R, d_t, d_status, d_cnt, d_h, d_rmse, d_info);
    HIPCHK(hipGetLastError());
    TRY(ransac_inlier_lists<ResectTask>(s, total, nj, d_tasks, d_status, ResectInlier{d_rec, d_R, d_t, intr[0], intr[1], o.max_error_px},
                            ResectEmit{d_tasks, nj}, capacity, inlier_off, inliers));
    HIPCHK(lvba::copy_d2h(Rcw, d_R, 72 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(tcw, d_t, 24 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(status, d_status, 4 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(n_inliers, d_cnt, 4 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(best_h, d_h, 4 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(rmse_px, d_rmse, 8 * (size_t)nj));
    HIPCHK(lvba::copy_d2h(information, d_info, 288 * (size_t)nj));
    return LVBA_OK;
}

extern "C" int32_t lvba_resect_hypotheses(int32_t device, int32_t id, int64_t n_corr, const float *uv, const double *world, const double *intr,
                                          const lvba_resect_opts *opts, double *R, double *t, int32_t *count)
{
    if (!intr || !R || !t || !count || n_corr < 0 || n_corr >= INT32_MAX || (n_corr > 0 && (!uv || !world)))
        return lvba_fail(LVBA_ERR_ARG, "null argument or n_corr out of range");
    if (id < 0) return lvba_fail(LVBA_ERR_ARG, "job id %d (>= 0)", id);
    lvba_resect_opts o;
    TRY(check_opts(opts, o));
    TRY(check_camera(intr));
    TRY(check_device(device));
    const size_t H = (size_t)o.hypotheses;
    if (n_corr < RESECT_K) { // no sample can be drawn: every hypothesis is invalid
        std::fill(R, R + 9 * H, 0.0);
        std::fill(t, t + 3 * H, 0.0);
        std::fill(count, count + H, -1);
        return LVBA_OK;
    }
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const int64_t off[2] = {0, n_corr};
    Records recs(sg.s);
    TRY(make_records(sg.s, device, 1, off, uv, world, intr, recs));
    std::vector<ResectTask> tasks(1);
    tasks[0] = ResectTask{};
    tasks[0].span.m = (int32_t)n_corr; tasks[0].id = id;
    DevArr<ResectTask> d_tasks(sg.s); DevArr<ResectBest> d_blk(sg.s); DevArr<double> d_pose(sg.s); DevArr<int32_t> d_c(sg.s);
    HIPCHK(d_pose.alloc(12 * H)); HIPCHK(d_c.alloc(H));
    TRY(run_hypotheses(sg.s, tasks, o, intr, recs.rec, d_tasks, d_blk, d_pose, d_c));
    std::vector<double> pose(12 * H);
    HIPCHK(d_pose.download(pose.data(), 12 * H));
    for (size_t h = 0; h < H; ++h) { std::copy_n(&pose[12 * h], 9, R + 9 * h); std::copy_n(&pose[12 * h + 9], 3, t + 3 * h); }
    HIPCHK(d_c.download(count, H));
    return LVBA_OK;
}

extern "C" int32_t lvba_resect_score(int32_t device, int64_t n_corr, const float *uv, const double *world, const double *intr, const double *Rcw,
                                     const double *tcw, double max_error_px, uint8_t *mask)
{
    if (!intr || !Rcw || !tcw || n_corr < 0 || n_corr >= INT32_MAX || (n_corr > 0 && (!uv || !world || !mask)))
        return lvba_fail(LVBA_ERR_ARG, "null argument or n_corr out of range");
    if (!(std::isfinite(max_error_px) && max_error_px > 0.0)) return lvba_fail(LVBA_ERR_ARG, "max_error_px %g (finite, > 0)", max_error_px);
    TRY(check_camera(intr));
    TRY(check_device(device));
    if (n_corr == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const int64_t off[2] = {0, n_corr};
    Records recs(sg.s);
    TRY(make_records(sg.s, device, 1, off, uv, world, intr, recs));
    ResectTask task{};
    task.span.m = (int32_t)n_corr;
    DevArr<double> d_pose(sg.s);
    HIPCHK(d_pose.alloc(12)); HIPCHK(d_pose.upload(Rcw, 9)); HIPCHK(copy_h2d(d_pose + 9, tcw, d_pose.bytes(3)));
    return ransac_score_mask(sg.s, task, ResectInlier{recs.rec, d_pose, d_pose + 9, intr[0], intr[1], max_error_px},
                             mask);
}

extern "C" int32_t lvba_resect_lift(lvba_depth_t depth, int32_t n_images, const int64_t *kp_off, const float *uv, const double *intr,
                                    const double *Rcw, const double *tcw, double *world)
{
    if (!depth || !kp_off || !intr || n_images < 0 || (n_images > 0 && (!Rcw || !tcw))) return lvba_fail(LVBA_ERR_ARG, "null argument or n_images < 0");
    if (depth->n_images != n_images) return lvba_fail(LVBA_ERR_ARG, "the depth set holds %d images, the call %d", depth->n_images, n_images);
    TRY(check_offsets("kp_off", "image", n_images, kp_off));
    TRY(check_camera(intr));
    TRY(check_rotations_finite(Rcw, 0, n_images));
    TRY(check_translations_finite(tcw, 0, n_images));
    const int64_t total = kp_off[n_images];
    if (total == 0) return LVBA_OK;
    if (!uv || !world) return lvba_fail(LVBA_ERR_ARG, "null keypoints or output");
    HIPCHK(hipSetDevice(depth->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    struct Guard { ImageSet set; ~Guard() { image_set_free(set); } } g;
    g.set = ImageSet{depth->device, n_images, std::vector<int64_t>(kp_off, kp_off + n_images + 1)};
    TRY(image_set_undistort(g.set, trk_intr_of(intr), uv, true));
    TRY(image_set_upload(g.set, true, nullptr));
    DevArr<double> d_w(sg.s), d_R(sg.s), d_t(sg.s);
    HIPCHK(d_w.alloc(3 * (size_t)total)); HIPCHK(d_R.alloc(9 * (size_t)n_images)); HIPCHK(d_t.alloc(3 * (size_t)n_images));
    HIPCHK(d_R.upload(Rcw, 9 * (size_t)n_images)); HIPCHK(d_t.upload(tcw, 3 * (size_t)n_images));
    resect_lift_kernel<<<grid_for(total, 256), 256, 0, sg.s>>>(total, n_images, g.set.d_off, g.set.d_uv, g.set.d_xy, depth->d_depth, depth->width,
                                                              depth->height, d_R, d_t, d_w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sg.s));
    HIPCHK(d_w.download(world, 3 * (size_t)total));
    return LVBA_OK;
}
