// register.hip -- scan-to-map registration: point-to-plane Gauss-Newton of a batch of (scan, initial pose) jobs against a voxel
// plane map -- or, job by job, against one submap of a submap set (lvba_register_*_submaps) --, in lock-step over the batch.  The per-point rule and the per-job step are register_device.h (also compiled for the
// host by the tests); the plane association is the map's own lookup (voxel_lookup.h); definitions in include/lvba_hip.h and
// DESIGN.md §10c.
//
// Device design, per iteration two launches and one word read by the host:
//   reg_linearize_kernel   grid (workgroups, jobs).  A job of m points uses nb = reg_blocks(m) workgroups -- a function of m alone, so
//                          a job's bytes do not depend on what else is in the batch --; lane l of workgroup b takes the points
//                          b * 256 + l + k * nb * 256, k = 0, 1, ...: coalesced 12-byte loads, the REG_NS sums stay in registers.
//                          The map tables (a few hundred roots and planes) are read through the caches.  Then a fixed tree: DPP row
//                          shifts and broadcasts inside each wavefront, the four wavefronts' shares added in index order through LDS,
//                          one partial [REG_NS] per workgroup.  No atomics: the bytes do not change run to run.
//   reg_step_kernel        one wavefront per job: lane q adds the job's partials of sum q in index order; lane 0 takes the
//                          eigenvalues of H / inliers (cyclic Jacobi, 6 x 6, in LDS), factorises H (LDL^T), decides the job's state
//                          and retracts the pose in place.  A job that goes on sets the iteration's word in the host's pinned
//                          memory; the lanes of a finished job return at once in both kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "voxel_lookup.h"
#include "wave_ops.h"
#include "register_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

static_assert(LVBA_REG_CONVERGED == REG_CONVERGED && LVBA_REG_MAX_ITERATIONS == REG_MAX_ITERATIONS &&
              LVBA_REG_TOO_FEW_INLIERS == REG_TOO_FEW && LVBA_REG_DEGENERATE == REG_DEGENERATE, "register states");

namespace {

constexpr int REG_BLOCK = 256;      // lanes of a linearisation workgroup
constexpr int REG_RUN = 8;          // points per lane up to REG_MAX_BLOCKS workgroups per job
constexpr int REG_MAX_BLOCKS = 64;

__host__ __device__ inline int reg_blocks(int64_t m)
{
    const int64_t nb = (m + (int64_t)REG_BLOCK * REG_RUN - 1) / ((int64_t)REG_BLOCK * REG_RUN);
    return (int)(nb < 1 ? 1 : nb > REG_MAX_BLOCKS ? REG_MAX_BLOCKS : nb);
}

// part [jobs][gridDim.x][REG_NS].  SUBMAPS = false: every job against the whole root table (submap unused; the single-map code
// as it was).  SUBMAPS = true: job k against submap[k] of a submap set: the job's root range is read once, from two uniform
// addresses, and stays in scalar registers.
template <bool SUBMAPS>
__global__ __launch_bounds__(REG_BLOCK) void reg_linearize_kernel(const VoxLookup map, const float *__restrict__ pts,
                                                                  const int64_t *__restrict__ frame_off, const int32_t *__restrict__ frames,
                                                                  const int32_t *__restrict__ submap, const double *__restrict__ poses,
                                                                  const lvba_register_result *__restrict__ res, const RegParams o,
                                                                  double *__restrict__ part)
{
    __shared__ double red[REG_BLOCK / 64][REG_NS];
    const int job = blockIdx.y;
    if (res[job].status != REG_RUNNING) return;
    const int f = frames[job];
    const int64_t p0 = frame_off[f], m = frame_off[f + 1] - p0;
    const int nb = reg_blocks(m);
    if ((int)blockIdx.x >= nb) return;
    int64_t r0 = 0, r1 = map.R;
    if (SUBMAPS && map.win_r0) {
        const int w = submap[job];
        r0 = map.win_r0[w];
        r1 = map.win_r0[w + 1];
    }
    double T[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) T[a] = poses[12 * (int64_t)job + a];
    double s[REG_NS];
#pragma unroll
    for (int q = 0; q < REG_NS; ++q) s[q] = 0.0;
    const float *P = pts + 3 * p0;
    for (int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; i < m; i += (int64_t)nb * REG_BLOCK) {
        const double p[3] = {(double)P[3 * i], (double)P[3 * i + 1], (double)P[3 * i + 2]};
        double w[3], pl[4];
        pose_apply(T, p[0], p[1], p[2], w);
        if (vox_find_plane(w, map.vs, r0, r1, map.root_key, map.mask, map.rootinfo, map.plane_first, map.plane, pl))
            reg_point(T, p, w, pl, o, s);
    }
#pragma unroll
    for (int q = 0; q < REG_NS; ++q) s[q] = wave_sum_to_lane63(s[q]); // (a lane without a source adds 0.0)
    // per component, from lane 63, for REG_NS threads to finish: not block_sum (wave_ops.h), which sums one value through lane 0
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < REG_NS; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < REG_NS) {
        const int q = threadIdx.x;
        part[((int64_t)job * gridDim.x + blockIdx.x) * REG_NS + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// stride: the linearisation's gridDim.x.  sums_only: lvba_register_linearize (no step).  sums [jobs][REG_NS] keeps the sums of
// the job's last linearisation.  flag: the host's word of this iteration, set by every job that goes on.
__global__ __launch_bounds__(64) void reg_step_kernel(int stride, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ frames,
                                                      const double *__restrict__ part, const RegParams o, int sums_only, int it, int max_it,
                                                      double *__restrict__ poses, lvba_register_result *__restrict__ res,
                                                      double *__restrict__ sums, int32_t *__restrict__ flag)
{
    __shared__ double sh[REG_NS];
    __shared__ double ws[REG_WS];
    const int job = blockIdx.x;
    if (res[job].status != REG_RUNNING) return;
    const int f = frames[job];
    const int nb = reg_blocks(frame_off[f + 1] - frame_off[f]);
    if (threadIdx.x < REG_NS) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += part[((int64_t)job * stride + b) * REG_NS + threadIdx.x];
        sh[threadIdx.x] = a;
        sums[(int64_t)job * REG_NS + threadIdx.x] = a;
    }
    __syncthreads();
    if (sums_only || threadIdx.x != 0) return;
    lvba_register_result &r = res[job];
    double min_eig, rmse;
    int st = reg_step(sh, o, poses + 12 * (int64_t)job, ws, &min_eig, &rmse);
    r.iterations = it + 1;
    r.inliers = (int64_t)sh[REG_CNT];
    r.cost_last = sh[REG_COST];
    if (it == 0) r.cost_first = sh[REG_COST];
    r.rmse = rmse;
    r.min_eigenvalue = min_eig;
    if (st == REG_RUNNING && it + 1 >= max_it) st = REG_MAX_ITERATIONS;
    if (st == REG_RUNNING) *flag = 1;
    else r.status = st;
}

int32_t check_opts(const lvba_register_opts *opts, lvba_register_opts &o, RegParams &p)
{
    lvba_register_default_opts(&o);
    if (opts) o = *opts;
    if (o.max_iterations < 1 || o.max_iterations > 1000 || !(o.max_distance > 0.0) || !std::isfinite(o.max_distance) || o.min_inliers < 0 ||
        !(o.min_eigenvalue >= 0.0) || !(o.tol_rot >= 0.0) || !(o.tol_pos >= 0.0))
        return lvba_fail(LVBA_ERR_ARG, "options: max_iterations %d (1 .. 1000), max_distance %g (> 0), min_inliers %lld, min_eigenvalue %g, "
                         "tol_rot %g, tol_pos %g (>= 0)", o.max_iterations, o.max_distance, (long long)o.min_inliers, o.min_eigenvalue,
                         o.tol_rot, o.tol_pos);
    if (o.loss.kind < LVBA_LOSS_TRIVIAL || o.loss.kind > LVBA_LOSS_TUKEY ||
        (o.loss.kind != LVBA_LOSS_TRIVIAL && !(o.loss.scale > 0.0 && std::isfinite(o.loss.scale))))
        return lvba_fail(LVBA_ERR_ARG, "loss: kind %d, scale %g (a known kind; finite and > 0 unless trivial)", o.loss.kind, o.loss.scale);
    p.max_distance = o.max_distance; p.min_eigenvalue = o.min_eigenvalue; p.tol_rot = o.tol_rot; p.tol_pos = o.tol_pos;
    p.loss_scale = o.loss.scale; p.min_inliers = o.min_inliers; p.loss_kind = o.loss.kind;
    return LVBA_OK;
}

// All entry points.  sums_only: one linearisation, H / g / cost / inliers out; else the iteration, poses_out / information /
// results out.  submaps: the map is a submap set and job k works against submap[k] (else a map of one window, submap unused).
int32_t reg_run(lvba_voxmap_t map, lvba_scans_t sc, int32_t n, const int32_t *frames, const int32_t *submap, bool submaps,
                const double *poses, const lvba_register_opts *opts, bool sums_only, double *H, double *g, double *cost, int64_t *inliers, double *poses_out, lvba_register_result *results)
{
    if (!map || !sc || n < 0) return lvba_fail(LVBA_ERR_ARG, "null map or scans, or n < 0");
    lvba_register_opts o;
    RegParams par;
    TRY(check_opts(opts, o, par));
    VoxLookup tab;
    int device = 0;
    TRY(submaps ? lvba_voxmap_lookup_tables_windows(map, &tab, &device) : lvba_voxmap_lookup_tables(map, &tab, &device));
    if (device != sc->device) return lvba_fail(LVBA_ERR_ARG, "the map is on device %d, the scans on device %d", device, sc->device);
    if (n == 0) return LVBA_OK;
    if (!frames || !poses || (submaps && !submap) || (sums_only ? !(H && g && cost && inliers) : !(poses_out && results)))
        return lvba_fail(LVBA_ERR_ARG, "null argument");
    int max_blocks = 1;
    for (int32_t k = 0; k < n; ++k) {
        if (frames[k] < 0 || frames[k] >= sc->n_frames) return lvba_fail(LVBA_ERR_ARG, "job %d: frame %d of %d", k, frames[k], sc->n_frames);
        if (submaps && (submap[k] < 0 || submap[k] >= tab.n_windows))
            return lvba_fail(LVBA_ERR_ARG, "job %d: submap %d of %d", k, submap[k], tab.n_windows);
        for (int a = 0; a < 12; ++a)
            if (!std::isfinite(poses[12 * (size_t)k + a])) return lvba_fail(LVBA_ERR_ARG, "job %d: non-finite pose", k);
        max_blocks = std::max(max_blocks, reg_blocks(sc->frame_off[frames[k] + 1] - sc->frame_off[frames[k]]));
    }
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    const int max_it = sums_only ? 1 : o.max_iterations;
    PinnedWords words;
    HIPCHK(PinnedCache::get().acquire((void **)&words.p, 4096)); // (>= 1000 words; one size for the cache's sake)
    int32_t *d_words = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&d_words, words.p, 0));
    for (int it = 0; it < max_it; ++it) words.p[it] = 0;
    std::vector<lvba_register_result> hres((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        hres[k] = lvba_register_result{};
        hres[k].status = REG_RUNNING;
        hres[k].points = sc->frame_off[frames[k] + 1] - sc->frame_off[frames[k]];
    }
    DevArr<int32_t> d_frames(s); DevArr<double> d_poses(s); DevArr<lvba_register_result> d_res(s);
    DevArr<double> d_part(s), d_sums(s); DevArr<int32_t> d_submap(s);
    if (submaps) {
        HIPCHK(d_submap.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(d_submap, submap, d_submap.bytes((size_t)n), hipMemcpyHostToDevice, s));
    }
    HIPCHK(d_frames.alloc((size_t)n)); HIPCHK(d_poses.alloc(12 * (size_t)n)); HIPCHK(d_res.alloc((size_t)n));
    HIPCHK(d_part.alloc((size_t)REG_NS * (size_t)max_blocks * (size_t)n)); HIPCHK(d_sums.alloc((size_t)REG_NS * (size_t)n));
    HIPCHK(hipMemcpyAsync(d_frames, frames, d_frames.bytes((size_t)n), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_poses, poses, d_poses.bytes(12 * (size_t)n), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_res, hres.data(), d_res.bytes((size_t)n), hipMemcpyHostToDevice, s));
    HIPCHK(d_sums.zero_async((size_t)REG_NS * (size_t)n));
    for (int it = 0; it < max_it; ++it) {
        (submaps ? reg_linearize_kernel<true> : reg_linearize_kernel<false>)<<<dim3((unsigned)max_blocks, (unsigned)n), REG_BLOCK, 0, s>>>(
            tab, sc->d_pts, sc->d_frame_off, d_frames, d_submap, d_poses, d_res, par,
            d_part);
        HIPCHK(hipGetLastError());
        reg_step_kernel<<<(unsigned)n, 64, 0, s>>>(max_blocks, sc->d_frame_off, d_frames, d_part, par, sums_only ? 1 : 0, it,
                                                   max_it, d_poses, d_res, d_sums, d_words + it);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        if (!words.p[it]) break; // every job has finished
    }
    std::vector<double> hsums((size_t)REG_NS * (size_t)n);
    HIPCHK(hipMemcpyAsync(hsums.data(), d_sums, d_sums.bytes(hsums.size()), hipMemcpyDeviceToHost, s));
    if (!sums_only) {
        HIPCHK(hipMemcpyAsync(poses_out, d_poses, d_poses.bytes(12 * (size_t)n), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(results, d_res, d_res.bytes((size_t)n), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int32_t k = 0; k < n; ++k) {
        const double *sk = hsums.data() + (size_t)REG_NS * k;
        reg_expand(sk, 1.0, H + 36 * (size_t)k);
        if (sums_only) {
            for (int a = 0; a < 6; ++a) g[6 * (size_t)k + a] = sk[REG_G0 + a];
            cost[k] = sk[REG_COST];
            inliers[k] = (int64_t)sk[REG_CNT];
        }
    }
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_register_default_opts(lvba_register_opts *o)
{
    if (!o) return;
    *o = lvba_register_opts{};
    o->max_iterations = 30;
    o->max_distance = 0.1;      // the fixture study
    o->min_inliers = 100;
    o->min_eigenvalue = 1e-3;
    o->tol_rot = 1e-6;
    o->tol_pos = 1e-6;
    o->loss.kind = LVBA_LOSS_TRIVIAL;
    o->loss.scale = 0.0;
}

extern "C" int32_t lvba_register_linearize(lvba_voxmap_t map, lvba_scans_t scans, int32_t n, const int32_t *frames, const double *poses,
                                           const lvba_register_opts *opts, double *H, double *g, double *cost, int64_t *inliers)
{
    return reg_run(map, scans, n, frames, nullptr, false, poses, opts, true, H, g, cost, inliers, nullptr, nullptr);
}

extern "C" int32_t lvba_register_scans(lvba_voxmap_t map, lvba_scans_t scans, int32_t n, const int32_t *frames, const double *poses_init,
                                       const lvba_register_opts *opts, double *poses_out, double *information,
                                       lvba_register_result *results)
{
    if (n > 0 && !information) return lvba_fail(LVBA_ERR_ARG, "null argument");
    return reg_run(map, scans, n, frames, nullptr, false, poses_init, opts, false, information, nullptr, nullptr, nullptr, poses_out, results);
}

extern "C" int32_t lvba_register_linearize_submaps(lvba_voxmap_t submaps, lvba_scans_t scans, int32_t n, const int32_t *frames,
                                                   const int32_t *submap, const double *poses, const lvba_register_opts *opts, double *H,
                                                   double *g, double *cost, int64_t *inliers)
{
    return reg_run(submaps, scans, n, frames, submap, true, poses, opts, true, H, g, cost, inliers, nullptr, nullptr);
}

extern "C" int32_t lvba_register_scans_submaps(lvba_voxmap_t submaps, lvba_scans_t scans, int32_t n, const int32_t *frames,
                                               const int32_t *submap, const double *poses_init, const lvba_register_opts *opts,
                                               double *poses_out, double *information, lvba_register_result *results)
{
    if (n > 0 && !information) return lvba_fail(LVBA_ERR_ARG, "null argument");
    return reg_run(submaps, scans, n, frames, submap, true, poses_init, opts, false, information, nullptr, nullptr, nullptr, poses_out,
                   results);
}
