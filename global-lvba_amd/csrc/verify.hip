// verify.hip -- two-view RANSAC over the putative matches of many image pairs at once (lvba_verify_*; the rule is in
// include/lvba_hip.h, its scalar pieces in verify_device.h).
//
// What is this stage's own, on the skeleton of ransac_batch.h (DESIGN.md §10k says which piece is whose):
//   (image_set.hip)           the undistorted keypoints: the handle's ImageSet, image_set_undistort once per handle.
//   verify_hypothesis_kernel  a lane draws its sample, reads those matches and solves; the eight-point method's 8 x 9 system lives in
//                             LDS, lane-interleaved, where the pivot search may index it at run time.  E then stays in nine register
//                             pairs; the same LDS stages the pair's match coordinates, 32 bytes each, in chunks of VERIFY_CHUNK,
//                             which every lane walks (a broadcast read) with match_device.h' gate.
//   verify_refine_kernel      a workgroup per pair: the sums over the winner's inliers (per-thread strides, then wave_ops.h' fixed
//                             trees), the refit in one lane (Jacobi on LDS), a rescore, kept only if the count grows; status.
//   VerifyInlier, VerifyEmit  the inlier test of the mask kernel; an inlier is written as its match, the caller's columns.
//   (the homography)          a third instantiation of the two kernels (METHOD = VERIFY_HOMOGRAPHY, no lvba_verify_opts::method): four
//                             matches fill the same 8 x 9 system, H and its inverse direction G stay in 18 register pairs, the scoring
//                             loop is the symmetric transfer test; VerifyInlierH is its mask.  lvba_verify_pairs_model's AUTO is a run
//                             under E, a run under H and the choice per pair on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "image_set.h"
#include "verify_device.h"
#include "ransac_batch.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

struct lvba_verify_s {
    ImageSet kp;                   // offsets on the host, undistorted points on the device
    bool has_R = false;
    std::vector<double> R;         // [n_images][9]
    double focal_sum = 0.0;        // fx + fy
};

namespace {

constexpr int VERIFY_CHUNK = 1024;          // matches staged in LDS at a time, 32 bytes each
constexpr int VERIFY_LDS_DOUBLES = 72 * RANSAC_HB > 4 * VERIFY_CHUNK ? 72 * RANSAC_HB : 4 * VERIFY_CHUNK;   // 36 864 bytes
constexpr int REFINE_BLOCK = 256;

struct VerifyTask {
    RansacSpan span;                // the pair's matches in the call's list, its block records
    int64_t lo_off, hi_off;         // first keypoint of lo and of hi
    int32_t lo, hi, swap;           // swap: the pair was given as (hi, lo), column 1 of its matches is the lo image
    double R[9];                    // R_hi R_lo^T (method 1)
};
typedef RansacBest<9> VerifyBest;   // the model is E

// the undistorted coordinates (x_lo, y_lo, x_hi, y_hi) of match i of the task
__device__ __forceinline__ void load_match(const VerifyTask &t, const int32_t *__restrict__ matches, const double *__restrict__ xy, int i,
                                           double &xl, double &yl, double &xh, double &yh)
{
    const int2 mm = reinterpret_cast<const int2 *>(matches)[t.span.off + i];
    const int64_t kl = t.lo_off + (t.swap ? mm.y : mm.x), kh = t.hi_off + (t.swap ? mm.x : mm.y);
    const double2 pl = reinterpret_cast<const double2 *>(xy)[kl], ph = reinterpret_cast<const double2 *>(xy)[kh];
    xl = pl.x; yl = pl.y; xh = ph.x; yh = ph.y;
}

// tiles [n_tiles]; blk, diag_E, diag_count: see ransac_block_best
template <int METHOD>
__global__ __launch_bounds__(RANSAC_HB) void verify_hypothesis_kernel(const VerifyTask *__restrict__ tasks, const RansacTile *__restrict__ tiles,
                                                                      const int32_t *__restrict__ matches, const double *__restrict__ xy,
                                                                      uint64_t seed, int H, double tau2, VerifyBest *__restrict__ blk,
                                                                      double *__restrict__ diag_E, int32_t *__restrict__ diag_count)
{
    constexpr int K = METHOD == VERIFY_KNOWN_ROTATION ? 2 : METHOD == VERIFY_HOMOGRAPHY ? 4 : 8;
    __shared__ __attribute__((aligned(16))) double lds[METHOD == VERIFY_KNOWN_ROTATION ? 4 * VERIFY_CHUNK : VERIFY_LDS_DOUBLES];
    const RansacLane ln = ransac_lane(tiles, H);
    const VerifyTask &t = tasks[ln.task];
    const int lane = threadIdx.x, m = t.span.m;
    double E[9], G[9];              // G: the homography's inverse direction, unused otherwise
    bool valid = false;
    verify_zero(E);
    verify_zero(G);
    if (ln.live) {
        int32_t idx[K];
        ransac_sample<K>(ransac_key(seed, t.lo, t.hi, ln.h), m, idx);
        if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
            bool clean = true;
            double xl0 = 0.0, yl0 = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double xl, yl, xh, yh;
                load_match(t, matches, xy, idx[j], xl, yl, xh, yh);
                clean &= verify_homography_rows(lds + lane, RANSAC_HB, j, xl, yl, xh, yh);
                if (j == 0) { xl0 = xl; yl0 = yl; }
            }
            valid = clean && verify_homography_solve(lds + lane, RANSAC_HB, xl0, yl0, E, G);
        } else if constexpr (METHOD == VERIFY_EIGHT_POINT) {
            bool clean = true;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double xl, yl, xh, yh;
                load_match(t, matches, xy, idx[j], xl, yl, xh, yh);
                clean &= verify_eight_row(lds + lane, RANSAC_HB, j, xl, yl, xh, yh);
            }
            valid = clean && verify_eight_solve(lds + lane, RANSAC_HB, E);
        } else {
            double p[8], R[9];
            load_match(t, matches, xy, idx[0], p[0], p[1], p[2], p[3]);
            load_match(t, matches, xy, idx[1], p[4], p[5], p[6], p[7]);
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = t.R[k];
            valid = verify_known_rotation(p, R, E);
        }
    }
    __syncthreads(); // the systems are done with: the same LDS now stages the matches
    int32_t count = 0;
    for (int c0 = 0; c0 < m; c0 += VERIFY_CHUNK) {
        const int n = min(VERIFY_CHUNK, m - c0);
        for (int i = lane; i < n; i += RANSAC_HB) {
            double xl, yl, xh, yh;
            load_match(t, matches, xy, c0 + i, xl, yl, xh, yh);
            lds[4 * i] = xl; lds[4 * i + 1] = yl; lds[4 * i + 2] = xh; lds[4 * i + 3] = yh;
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const double2 pl = reinterpret_cast<const double2 *>(lds)[2 * i], ph = reinterpret_cast<const double2 *>(lds)[2 * i + 1];
            if constexpr (METHOD == VERIFY_HOMOGRAPHY) count += verify_inlier_h(E, G, pl.x, pl.y, ph.x, ph.y, tau2) ? 1 : 0;
            else count += verify_inlier(E, pl.x, pl.y, ph.x, ph.y, tau2) ? 1 : 0;
        }
        __syncthreads();
    }
    if (!valid) count = -1;
    ransac_block_best<9>(ln, count, E, blk, diag_E, diag_count);
}

// E [P][9], status, n_inliers, best_h [P]: the pair's result after `rounds` refits
template <int METHOD>
__global__ __launch_bounds__(REFINE_BLOCK) void verify_refine_kernel(const VerifyTask *__restrict__ tasks, const int32_t *__restrict__ matches,
                                                                     const double *__restrict__ xy, double tau2, int rounds, int min_inliers,
                                                                     const VerifyBest *__restrict__ res, double *__restrict__ E_out,
                                                                     int32_t *__restrict__ status, int32_t *__restrict__ n_inliers,
                                                                     int32_t *__restrict__ best_h)
{
    constexpr int NS = METHOD == VERIFY_KNOWN_ROTATION ? 6 : 45;
    constexpr int WAVES = REFINE_BLOCK / 64;
    __shared__ double red[WAVES];
    __shared__ double sT[NS], sN[81], sV[81], sE[METHOD == VERIFY_HOMOGRAPHY ? 18 : 9];   // the homography: H, then G
    __shared__ int s_ok;
    const int p = blockIdx.x, tid = threadIdx.x;
    const VerifyTask &t = tasks[p];
    const int m = t.span.m;
    const VerifyBest b = res[p];
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = b.model[k];
    int32_t count = b.count;
    double G[9];                    // the homography's inverse direction, unused otherwise
    if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
        if (!verify_homography_inverse(E, G)) count = count > 0 ? 0 : count;   // never of a winner: its G existed in the hypothesis kernel
    }
    const auto inlier = [tau2](const double *M, const double *Mi, double xl, double yl, double xh, double yh) {
        if constexpr (METHOD == VERIFY_HOMOGRAPHY) return verify_inlier_h(M, Mi, xl, yl, xh, yh, tau2);
        else return verify_inlier(M, xl, yl, xh, yh, tau2);
    };
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = t.R[k];
    for (int round = 0; round < rounds && count > 0; ++round) { // every condition below is the same in all threads
        double acc[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) acc[k] = 0.0;
        for (int i = tid; i < m; i += REFINE_BLOCK) {
            double xl, yl, xh, yh;
            load_match(t, matches, xy, i, xl, yl, xh, yh);
            if (!inlier(E, G, xl, yl, xh, yh)) continue;
            if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
                double r1[9], r2[9];
                verify_homography_row_pair(xl, yl, xh, yh, r1, r2);
                int k = 0;
#pragma unroll
                for (int r = 0; r < 9; ++r)
#pragma unroll
                    for (int c = r; c < 9; ++c) acc[k++] += r1[r] * r1[c] + r2[r] * r2[c];
            } else if constexpr (METHOD == VERIFY_EIGHT_POINT) {
                const double a[9] = {xh * xl, xh * yl, xh, yh * xl, yh * yl, yh, xl, yl, 1.0};
                int k = 0;
#pragma unroll
                for (int r = 0; r < 9; ++r)
#pragma unroll
                    for (int c = r; c < 9; ++c) acc[k++] += a[r] * a[c];
            } else {
                double c[3];
                verify_constraint(R, xl, yl, xh, yh, c);
                acc[0] += c[0] * c[0]; acc[1] += c[0] * c[1]; acc[2] += c[0] * c[2];
                acc[3] += c[1] * c[1]; acc[4] += c[1] * c[2]; acc[5] += c[2] * c[2];
            }
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double sum = block_sum_all<WAVES>(acc[k], red);
            if (tid == 0) sT[k] = sum;
        }
        if (tid == 0) {
            double F[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = E[k];
            bool ok;
            if constexpr (METHOD != VERIFY_KNOWN_ROTATION) {
                int k = 0;
#pragma unroll
                for (int r = 0; r < 9; ++r)
#pragma unroll
                    for (int c = r; c < 9; ++c) { sN[9 * r + c] = sT[k]; sN[9 * c + r] = sT[k]; ++k; }
                if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
                    double Gf[9];
                    ok = verify_refit_homography(sN, sV, F, Gf);
#pragma unroll
                    for (int k2 = 0; k2 < 9; ++k2) sE[9 + k2] = Gf[k2];
                } else {
                    ok = verify_refit_eight(sN, sV, F);
                }
            } else {
                double C[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) C[k] = sT[k];
                ok = verify_refit_rotation(C, R, F);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) sE[k] = F[k];
            s_ok = ok ? 1 : 0;
        }
        __syncthreads();
        const bool ok = s_ok != 0;
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = sE[k];
        double Gf[9];
        if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
#pragma unroll
            for (int k = 0; k < 9; ++k) Gf[k] = sE[9 + k];
        }
        __syncthreads(); // sE and s_ok are free again
        if (!ok) break;
        int32_t c = 0;
        for (int i = tid; i < m; i += REFINE_BLOCK) {
            double xl, yl, xh, yh;
            load_match(t, matches, xy, i, xl, yl, xh, yh);
            c += inlier(F, Gf, xl, yl, xh, yh) ? 1 : 0;
        }
        const int32_t cn = (int32_t)block_sum_all<WAVES>((double)c, red); // integers below 2^31: exact in fp64 in any order
        if (cn <= count) break;                                           // kept only if strictly better
        count = cn;
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = F[k];
        if constexpr (METHOD == VERIFY_HOMOGRAPHY) {
#pragma unroll
            for (int k = 0; k < 9; ++k) G[k] = Gf[k];
        }
    }
    if (tid != 0) return;
    status[p] = ransac_status(m, verify_sample_size(METHOD), min_inliers, count);
    n_inliers[p] = count > 0 ? count : 0;
    best_h[p] = b.h;
#pragma unroll
    for (int k = 0; k < 9; ++k) E_out[9 * (int64_t)p + k] = E[k];
}

// match i of the call, of pair j, is an inlier of E [j]
struct VerifyInlier {
    const int32_t *matches;
    const double *xy, *E;
    double tau2;
    __device__ bool operator()(const VerifyTask &t, int j, int64_t i) const
    {
        double xl, yl, xh, yh;
        load_match(t, matches, xy, (int)(i - t.span.off), xl, yl, xh, yh);
        return verify_inlier(E + 9 * (int64_t)j, xl, yl, xh, yh, tau2);
    }
};
// match i of the call, of pair j, is an inlier of the homography H [j] and of its inverse direction
struct VerifyInlierH {
    const int32_t *matches;
    const double *xy, *H;
    double tau2;
    __device__ bool operator()(const VerifyTask &t, int j, int64_t i) const
    {
        double xl, yl, xh, yh, Hj[9], G[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Hj[k] = H[9 * (int64_t)j + k];
        if (!verify_homography_inverse(Hj, G)) return false;
        load_match(t, matches, xy, (int)(i - t.span.off), xl, yl, xh, yh);
        return verify_inlier_h(Hj, G, xl, yl, xh, yh, tau2);
    }
};
// an inlier is its match, the caller's columns
struct VerifyEmit {
    static constexpr int WIDTH = 2;
    const int32_t *matches;
    __device__ void operator()(int32_t *out, int64_t pos, int64_t i) const { out[2 * pos] = matches[2 * i]; out[2 * pos + 1] = matches[2 * i + 1]; }
};

int32_t check_opts(const lvba_verify_s *v, const lvba_verify_opts *opts, lvba_verify_opts &o)
{
    lvba_verify_default_opts(&o);
    if (opts) o = *opts;
    if (o.method != VERIFY_EIGHT_POINT && o.method != VERIFY_KNOWN_ROTATION) return lvba_fail(LVBA_ERR_ARG, "method %d (0 or 1)", o.method);
    if (o.hypotheses < 1) return lvba_fail(LVBA_ERR_ARG, "hypotheses %d (>= 1)", o.hypotheses);
    if (o.refine_rounds < 0 || o.min_inliers < 0 || !(std::isfinite(o.max_error_px) && o.max_error_px > 0.0))
        return lvba_fail(LVBA_ERR_ARG, "options: refine_rounds %d (>= 0), min_inliers %d (>= 0), max_error_px %g (finite, > 0)", o.refine_rounds,
                         o.min_inliers, o.max_error_px);
    if (o.method == VERIFY_KNOWN_ROTATION && !v->has_R)
        return lvba_fail(LVBA_ERR_ARG, "the rotation-aided method (method = 1) needs the rotations Rcw at lvba_verify_create");
    return LVBA_OK;
}

// the task of pair (a, b) with matches [m_off, m_off + m) of `matches`, every index checked
int32_t make_task(const lvba_verify_s *v, int64_t a, int64_t b, int64_t m_off, int64_t m, const int32_t *matches, int method, VerifyTask &t)
{
    TRY(check_image_pair(a, b, v->kp.n_images));
    if (m < 0 || m >= INT32_MAX) return lvba_fail(LVBA_ERR_ARG, "pair (%lld, %lld) with %lld matches", (long long)a, (long long)b, (long long)m);
    const int64_t n_a = v->kp.off[a + 1] - v->kp.off[a], n_b = v->kp.off[b + 1] - v->kp.off[b];
    for (int64_t i = m_off; i < m_off + m; ++i)
        if (matches[2 * i] < 0 || matches[2 * i] >= n_a || matches[2 * i + 1] < 0 || matches[2 * i + 1] >= n_b)
            return lvba_fail(LVBA_ERR_ARG, "match %lld = (%d, %d) of pair (%lld, %lld) with %lld and %lld keypoints", (long long)i, matches[2 * i],
                             matches[2 * i + 1], (long long)a, (long long)b, (long long)n_a, (long long)n_b);
    t = VerifyTask{};
    t.lo = (int32_t)std::min(a, b); t.hi = (int32_t)std::max(a, b); t.swap = a > b ? 1 : 0;
    t.lo_off = v->kp.off[t.lo]; t.hi_off = v->kp.off[t.hi]; t.span.off = m_off; t.span.m = (int32_t)m;
    if (method == VERIFY_KNOWN_ROTATION) verify_relative_rotation(&v->R[9 * (size_t)t.lo], &v->R[9 * (size_t)t.hi], t.R);
    return LVBA_OK;
}

// The hypotheses of every pair with enough matches (ransac_run_hypotheses).  diag_E, diag_count: null, or the diagnostic call's outputs.
// method: o.method, or VERIFY_HOMOGRAPHY.
int32_t run_hypotheses(hipStream_t s, const lvba_verify_s *v, std::vector<VerifyTask> &tasks, const lvba_verify_opts &o, int method,
                       const int32_t *d_matches, DevArr<VerifyTask> &d_tasks, DevArr<VerifyBest> &d_blk, double *diag_E, int32_t *diag_count)
{
    const int k = verify_sample_size(method);
    const double tau2 = match_tau2(v->focal_sum, o.max_error_px);
    const auto kernel = method == VERIFY_EIGHT_POINT    ? verify_hypothesis_kernel<VERIFY_EIGHT_POINT>
                        : method == VERIFY_HOMOGRAPHY ? verify_hypothesis_kernel<VERIFY_HOMOGRAPHY>
                                                      : verify_hypothesis_kernel<VERIFY_KNOWN_ROTATION>;
    return ransac_run_hypotheses<9>(s, tasks, o.hypotheses, diag_E ? k : std::max(k, o.min_inliers), d_tasks, d_blk, [&](unsigned grid, const RansacTile *tiles) {
        kernel<<<grid, RANSAC_HB, 0, s>>>(d_tasks, tiles, d_matches, v->kp.d_xy, o.seed, o.hypotheses, tau2, d_blk, diag_E,
                                          diag_count);
    });
}

} // namespace

extern "C" void lvba_verify_default_opts(lvba_verify_opts *o)
{
    if (!o) return;
    *o = lvba_verify_opts{};
    o->method = VERIFY_EIGHT_POINT; o->hypotheses = 1024; o->refine_rounds = 2; o->min_inliers = 15; o->max_error_px = 4.0; o->seed = 0;
}

extern "C" int32_t lvba_verify_create(int32_t device, int32_t n_images, const int64_t *kp_off, const float *keypoints_uv, const double *intr,
                                      const double *Rcw, lvba_verify_t *out)
{
    if (!out || n_images < 0 || !kp_off || !intr) return lvba_fail(LVBA_ERR_ARG, "null argument or n_images < 0");
    TRY(check_offsets("kp_off", "image", n_images, kp_off));
    const int64_t total = kp_off[n_images];
    if (total > 0 && !keypoints_uv) return lvba_fail(LVBA_ERR_ARG, "null keypoints");
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    if (Rcw) TRY(check_rotations_finite(Rcw, 0, n_images));
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_verify_s *v = new lvba_verify_s;
    v->kp = ImageSet{device, n_images, std::vector<int64_t>(kp_off, kp_off + n_images + 1)};
    v->focal_sum = intr[0] + intr[1];
    if (Rcw) { v->R.assign(Rcw, Rcw + 9 * (size_t)n_images); v->has_R = true; }
    const int32_t rc = image_set_undistort(v->kp, trk_intr_of(intr), keypoints_uv, false); // the pixels: on the device for this call only
    if (rc != LVBA_OK) { lvba_verify_destroy(v); return rc; }
    *out = v;
    return LVBA_OK;
}

extern "C" int32_t lvba_verify_destroy(lvba_verify_t v)
{
    if (!v) return LVBA_OK;
    (void)hipSetDevice(v->kp.device);
    (void)hipDeviceSynchronize();
    image_set_free(v->kp);
    delete v;
    return LVBA_OK;
}

namespace {

int32_t check_pairs_args(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, int64_t capacity, const int64_t *inlier_off,
                         const int32_t *inliers, const double *E, const int32_t *status, const int32_t *n_inliers, const int32_t *best_h)
{
    if (!v || !match_off || !inlier_off || n_pairs < 0 || capacity < 0 || (n_pairs > 0 && (!pairs || !E || !status || !n_inliers || !best_h)) ||
        (capacity > 0 && !inliers))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_pairs < 0 or capacity < 0");
    return LVBA_OK;
}

// lvba_verify_pairs under `method`: o.method, or VERIFY_HOMOGRAPHY (then E holds H).  The arguments and options are checked already.
int32_t run_pairs(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                  const lvba_verify_opts &o, int method, int64_t capacity, int64_t *inlier_off, int32_t *inliers, double *E, int32_t *status,
                  int32_t *n_inliers, int32_t *best_h)
{
    if (n_pairs >= INT32_MAX / 2) return lvba_fail(LVBA_ERR_UNSUPPORTED, "%lld pairs in one call", (long long)n_pairs);
    TRY(check_offsets("match_off", "pair", n_pairs, match_off));
    const int64_t total = match_off[n_pairs];
    if (total >= RANSAC_MAX_ELEMENTS) return lvba_fail(LVBA_ERR_UNSUPPORTED, "%lld matches in one call (below 2^31)", (long long)total);
    if (total > 0 && !matches) return lvba_fail(LVBA_ERR_ARG, "null matches");
    std::vector<VerifyTask> tasks((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p)
        TRY(make_task(v, pairs[2 * p], pairs[2 * p + 1], match_off[p], match_off[p + 1] - match_off[p], matches, method, tasks[(size_t)p]));
    inlier_off[0] = 0;
    if (n_pairs == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(v->kp.device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    hipStream_t s = sg.s;
    const int np = (int)n_pairs;
    const double tau2 = match_tau2(v->focal_sum, o.max_error_px);
    DevArr<int32_t> d_m(s); DevArr<VerifyTask> d_tasks(s); DevArr<VerifyBest> d_blk(s), d_res(s); DevArr<double> d_E(s);
    DevArr<int32_t> d_int(s);
    HIPCHK(d_m.alloc(2 * (size_t)total));
    if (total > 0) HIPCHK(d_m.upload(matches, 2 * (size_t)total));
    TRY(run_hypotheses(s, v, tasks, o, method, d_m, d_tasks, d_blk, nullptr, nullptr));
    HIPCHK(d_res.alloc((size_t)np)); HIPCHK(d_E.alloc(9 * (size_t)np)); HIPCHK(d_int.alloc(3 * (size_t)np));
    int32_t *d_status = d_int, *d_cnt = d_status + np, *d_h = d_cnt + np;
    ransac_pick_kernel<9, VerifyTask><<<grid_for(np, 256), 256, 0, s>>>(np, d_tasks, d_blk, d_res);
    HIPCHK(hipGetLastError());
    const auto refine = method == VERIFY_EIGHT_POINT    ? verify_refine_kernel<VERIFY_EIGHT_POINT>
                        : method == VERIFY_HOMOGRAPHY ? verify_refine_kernel<VERIFY_HOMOGRAPHY>
                                                      : verify_refine_kernel<VERIFY_KNOWN_ROTATION>;
    refine<<<(unsigned)np, REFINE_BLOCK, 0, s>>>(d_tasks, d_m, v->kp.d_xy, tau2, o.refine_rounds, o.min_inliers, d_res, d_E,
                                                 d_status, d_cnt, d_h);
    HIPCHK(hipGetLastError());
    if (method == VERIFY_HOMOGRAPHY)
        TRY(ransac_inlier_lists<VerifyTask>(s, total, np, d_tasks, d_status, VerifyInlierH{d_m, v->kp.d_xy, d_E, tau2},
                                VerifyEmit{d_m}, capacity, inlier_off, inliers));
    else
        TRY(ransac_inlier_lists<VerifyTask>(s, total, np, d_tasks, d_status, VerifyInlier{d_m, v->kp.d_xy, d_E, tau2},
                                VerifyEmit{d_m}, capacity, inlier_off, inliers));
    HIPCHK(d_E.download(E, 9 * (size_t)np));
    HIPCHK(lvba::copy_d2h(status, d_status, 4 * (size_t)np));
    HIPCHK(lvba::copy_d2h(n_inliers, d_cnt, 4 * (size_t)np));
    HIPCHK(lvba::copy_d2h(best_h, d_h, 4 * (size_t)np));
    return LVBA_OK;
}

// lvba_verify_hypotheses under `method`: o.method, or VERIFY_HOMOGRAPHY.  The options are checked already.
int32_t run_diagnostic(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const lvba_verify_opts &o, int method,
                       double *E, int32_t *count)
{
    std::vector<VerifyTask> tasks(1);
    TRY(make_task(v, a, b, 0, n_matches, matches, method, tasks[0]));
    const size_t H = (size_t)o.hypotheses;
    if (n_matches < verify_sample_size(method)) { // no sample can be drawn: every hypothesis is invalid
        std::fill(E, E + 9 * H, 0.0);
        std::fill(count, count + H, -1);
        return LVBA_OK;
    }
    HIPCHK(hipSetDevice(v->kp.device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<int32_t> d_m(sg.s); DevArr<VerifyTask> d_tasks(sg.s); DevArr<VerifyBest> d_blk(sg.s); DevArr<double> d_E(sg.s); DevArr<int32_t> d_c(sg.s);
    HIPCHK(d_m.alloc(2 * (size_t)n_matches)); HIPCHK(d_E.alloc(9 * H)); HIPCHK(d_c.alloc(H));
    HIPCHK(d_m.upload(matches, 2 * (size_t)n_matches));
    TRY(run_hypotheses(sg.s, v, tasks, o, method, d_m, d_tasks, d_blk, d_E, d_c)); HIPCHK(d_E.download(E, 9 * H));
    HIPCHK(d_c.download(count, H));
    return LVBA_OK;
}

// lvba_verify_score under the essential matrix (homography false) or the homography M
int32_t run_score(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const double *E, double max_error_px,
                  uint8_t *mask, bool homography)
{
    if (!v || !E || n_matches < 0 || (n_matches > 0 && (!matches || !mask))) return lvba_fail(LVBA_ERR_ARG, "null argument or n_matches < 0");
    if (!(std::isfinite(max_error_px) && max_error_px > 0.0)) return lvba_fail(LVBA_ERR_ARG, "max_error_px %g (finite, > 0)", max_error_px);
    std::vector<VerifyTask> tasks(1);
    TRY(make_task(v, a, b, 0, n_matches, matches, VERIFY_EIGHT_POINT, tasks[0]));
    if (n_matches == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(v->kp.device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<int32_t> d_m(sg.s); DevArr<double> d_E(sg.s);
    HIPCHK(d_m.alloc(2 * (size_t)n_matches)); HIPCHK(d_E.alloc(9)); HIPCHK(d_m.upload(matches, 2 * (size_t)n_matches));
    HIPCHK(d_E.upload(E, 9));
    const double tau2 = match_tau2(v->focal_sum, max_error_px);
    if (homography) return ransac_score_mask(sg.s, tasks[0], VerifyInlierH{d_m, v->kp.d_xy, d_E, tau2}, mask);
    return ransac_score_mask(sg.s, tasks[0], VerifyInlier{d_m, v->kp.d_xy, d_E, tau2}, mask);
}

// the options of a call that runs the homography alone: `method` is not read
int32_t check_opts_homography(const lvba_verify_s *v, const lvba_verify_opts *opts, lvba_verify_opts &o)
{
    lvba_verify_opts in;
    lvba_verify_default_opts(&in);
    if (opts) in = *opts;
    in.method = VERIFY_EIGHT_POINT;
    return check_opts(v, &in, o);
}

} // namespace

extern "C" int32_t lvba_verify_pairs(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                                     const lvba_verify_opts *opts, int64_t capacity, int64_t *inlier_off, int32_t *inliers, double *E,
                                     int32_t *status, int32_t *n_inliers, int32_t *best_h)
{
    TRY(check_pairs_args(v, n_pairs, pairs, match_off, capacity, inlier_off, inliers, E, status, n_inliers, best_h));
    lvba_verify_opts o;
    TRY(check_opts(v, opts, o));
    return run_pairs(v, n_pairs, pairs, match_off, matches, o, o.method, capacity, inlier_off, inliers, E, status, n_inliers, best_h);
}

extern "C" int32_t lvba_verify_hypotheses(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches,
                                          const lvba_verify_opts *opts, double *E, int32_t *count)
{
    if (!v || !E || !count || n_matches < 0 || (n_matches > 0 && !matches)) return lvba_fail(LVBA_ERR_ARG, "null argument or n_matches < 0");
    lvba_verify_opts o;
    TRY(check_opts(v, opts, o));
    return run_diagnostic(v, a, b, n_matches, matches, o, o.method, E, count);
}

extern "C" int32_t lvba_verify_score(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const double *E,
                                     double max_error_px, uint8_t *mask)
{
    return run_score(v, a, b, n_matches, matches, E, max_error_px, mask, false);
}

extern "C" int32_t lvba_verify_hypotheses_homography(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches,
                                                     const lvba_verify_opts *opts, double *Hm, int32_t *count)
{
    if (!v || !Hm || !count || n_matches < 0 || (n_matches > 0 && !matches)) return lvba_fail(LVBA_ERR_ARG, "null argument or n_matches < 0");
    lvba_verify_opts o;
    TRY(check_opts_homography(v, opts, o));
    return run_diagnostic(v, a, b, n_matches, matches, o, VERIFY_HOMOGRAPHY, Hm, count);
}

extern "C" int32_t lvba_verify_score_homography(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const double *Hm,
                                                double max_error_px, uint8_t *mask)
{
    return run_score(v, a, b, n_matches, matches, Hm, max_error_px, mask, true);
}

extern "C" int32_t lvba_verify_pairs_model(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                                           const lvba_verify_opts *opts, int32_t model, double planar_ratio, int64_t capacity, int64_t *inlier_off,
                                           int32_t *inliers, double *M, int32_t *kind, int32_t *status, int32_t *n_inliers, int32_t *best_h,
                                           int32_t *n_inliers_E, int32_t *n_inliers_H)
{
    TRY(check_pairs_args(v, n_pairs, pairs, match_off, capacity, inlier_off, inliers, M, status, n_inliers, best_h));
    if (n_pairs > 0 && !kind) return lvba_fail(LVBA_ERR_ARG, "null kind");
    if (model != VERIFY_MODEL_ESSENTIAL && model != VERIFY_MODEL_HOMOGRAPHY && model != VERIFY_MODEL_AUTO)
        return lvba_fail(LVBA_ERR_ARG, "model %d (0 essential, 1 homography, 2 auto)", model);
    if (!(std::isfinite(planar_ratio) && planar_ratio > 0.0)) return lvba_fail(LVBA_ERR_ARG, "planar_ratio %g (finite, > 0)", planar_ratio);
    lvba_verify_opts o;
    if (model == VERIFY_MODEL_HOMOGRAPHY) TRY(check_opts_homography(v, opts, o));
    else TRY(check_opts(v, opts, o));
    const size_t np = (size_t)n_pairs;
    if (model != VERIFY_MODEL_AUTO) {
        const bool h = model == VERIFY_MODEL_HOMOGRAPHY;
        TRY(run_pairs(v, n_pairs, pairs, match_off, matches, o, h ? VERIFY_HOMOGRAPHY : o.method, capacity, inlier_off, inliers, M, status, n_inliers,
                      best_h));
        for (size_t p = 0; p < np; ++p) {
            kind[p] = model;
            if (n_inliers_E) n_inliers_E[p] = h ? -1 : n_inliers[p];
            if (n_inliers_H) n_inliers_H[p] = h ? n_inliers[p] : -1;
        }
        return LVBA_OK;
    }
    // AUTO: both runs to completion with room for every inlier, the decision per pair on the host, the chosen run's outputs copied
    struct Run {
        std::vector<int64_t> off;
        std::unique_ptr<int32_t[]> inl;          // [total][2], not initialised: only [0, off[n_pairs]) is ever read
        std::vector<int32_t> status, n, h;
        std::vector<double> M;
    } run[2];
    TRY(check_offsets("match_off", "pair", n_pairs, match_off));
    const int64_t total = match_off[n_pairs];
    for (int k = 0; k < 2; ++k) {
        Run &r = run[k];
        r.off.resize(np + 1); r.inl.reset(new int32_t[2 * (size_t)std::max<int64_t>(total, 1)]); r.status.resize(np); r.n.resize(np); r.h.resize(np); r.M.resize(9 * np);
        TRY(run_pairs(v, n_pairs, pairs, match_off, matches, o, k ? VERIFY_HOMOGRAPHY : o.method, total, r.off.data(), r.inl.get(), r.M.data(),
                      r.status.data(), r.n.data(), r.h.data()));
    }
    int64_t pos = 0;
    inlier_off[0] = 0;
    for (size_t p = 0; p < np; ++p) {
        const int k = verify_choose_model(run[0].status[p], run[0].n[p], run[1].status[p], run[1].n[p], planar_ratio);
        const Run &r = run[k];
        kind[p] = k; status[p] = r.status[p]; n_inliers[p] = r.n[p]; best_h[p] = r.h[p];
        std::copy(r.M.begin() + 9 * p, r.M.begin() + 9 * p + 9, M + 9 * p);
        if (n_inliers_E) n_inliers_E[p] = run[0].n[p];
        if (n_inliers_H) n_inliers_H[p] = run[1].n[p];
        const int64_t n = r.off[p + 1] - r.off[p], room = std::min(n, std::max<int64_t>(capacity - pos, 0));
        if (room > 0) std::memcpy(inliers + 2 * pos, r.inl.get() + 2 * r.off[p], 8 * (size_t)room);
        pos += n;
        inlier_off[p + 1] = pos;
    }
    return LVBA_OK;
}
