// match.hip -- descriptor matching of image pairs with an optional pose-guided gate, on the epipolar line or at the point a LiDAR
// depth image predicts (lvba_match_*; the rule is in include/lvba_hip.h, its scalar pieces in match_device.h).
//
// Device design:
//   (image_set.hip)         pixels, offsets, undistorted points: the handle's ImageSet, image_set_undistort per set_geometry.
//   match_lift_kernel       a thread per keypoint: its 3-D point through the depth image, once per lvba_match_set_depth, NaN where
//                           it has none.
//   match_predict_kernel    depth gate only, before the scan: a thread per (ordered pair, keypoint of its first image) projects the
//                           keypoint's point into the second image -- for both orientations of every pair of the grid, since the scan
//                           of (a, b) needs a's keypoints in b for its rows and b's in a for its columns.  NaN: no point; +inf: the
//                           point does not project.
//   match_scan_kernel       the top two of every row of an ordered pair (a, b), for a whole list of ordered pairs in one grid.  A
//                           workgroup is four wavefronts, each with 32 rows of image a; its A fragments of all four k-steps stay in
//                           registers.  Column tiles of 32 descriptors of b stream through v_mfma_i32_32x32x32_i8; the accumulator
//                           starts at the column's bias 128 sum b', so that the biased score sum a'b' + 128 sum b' orders the columns
//                           of a row as the true score does (the rest of the identity is a per-row constant, added once at the end).
//                           Each lane keeps (s1, best, s2) for its 16 rows over the columns it sees -- a lane sees ascending columns,
//                           so a strict > keeps the lowest column of a tie -- and the 32 lanes of a row merge once at the end.  The
//                           n_a x n_b scores never leave the registers.  Under the gate a lane holds the epipolar line (or the
//                           point) of its 16 rows from the prologue on, computes its column's once per tile, and a candidate that
//                           fails is replaced by "none" before the update.  Under the depth gate it holds each row's pixel and
//                           prediction instead and loads its column's pixel and prediction once per tile.
//   match_decide_kernel     a thread per forward row: the fp64 acos clauses and the mutual clause -> a flag.
//   match_write_kernel      after an exclusive prefix sum of the flags: the matches in (pair, row) order, and match_off.
// The byte k of a descriptor that a lane feeds into a k-step is the same for the A and the B operand (bytes 64 h + 16 ks .. + 15 of
// lane half h), so the sum over k is complete whatever order the instruction takes them in.
// No atomics of any kind: two calls give the same bytes.
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
#include "../../include/lvba_hip.h"

using namespace lvba;

struct lvba_match_s {
    ImageSet kp;                   // offsets (on the device for the lift), pixels, undistorted points
    uint8_t *d_desc = nullptr;     // [total][128], top bit flipped: a' = a - 128 as a signed byte
    int32_t *d_bias = nullptr;     // [total] 128 sum a'
    double *d_pts = nullptr;       // [total][3] the keypoints' points through the depth images, NaN rows where there is none
    bool has_geometry = false, has_points = false;
    TrkIntr cam{};
    std::vector<double> R, t;      // [n_images][9], [n_images][3]
    double focal_sum = 0.0;        // fx + fy
};

namespace {

constexpr int SCAN_BLOCK = 256;             // four wavefronts, 32 rows each
constexpr int SCAN_ROWS = 32 * (SCAN_BLOCK / 64);
constexpr int64_t MATCH_MAX_PER_IMAGE = 1 << 20;
constexpr int64_t CHUNK_ROWS = (int64_t)1 << 23; // scanned rows per grid: 96 MB of top-two results

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct MatchTask {
    int64_t a_off, b_off, out_off;  // first descriptor of a and of b, first result row
    int32_t n_a, n_b;
    int32_t rows_lo, pad;           // 1: image a is the "lo" image of the gate
    union {
        double E[9];                // epipolar gate: lo -> hi
        struct { int64_t rows, cols; } pred; // depth gate: the first prediction of a's keypoints in b and of b's in a
    };
};

// keypoints [src_off, src_off + n) (one image) projected into the image with pose (R, t); predictions [first, first + n)
struct MatchPredJob {
    int64_t src_off, first;
    double R[9], t[3];
};

// world [n][3]; img_off [n_images + 1] = the matcher's desc_off
__global__ __launch_bounds__(256) void match_lift_kernel(int64_t n, int n_images, const int64_t *__restrict__ img_off,
                                                         const float *__restrict__ uv, const double *__restrict__ xy,
                                                         const float *__restrict__ depth, int width, int height,
                                                         const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                         double *__restrict__ world)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int lo = segment_of(img_off, n_images, i);
    match_lift(depth + (int64_t)lo * width * height, width, height, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1], Rcw + 9 * (int64_t)lo,
               tcw + 3 * (int64_t)lo, world + 3 * i);
}

// pred [n][2]; jobs by ascending `first`, none empty
__global__ __launch_bounds__(256) void match_predict_kernel(int64_t n, int n_jobs, const MatchPredJob *__restrict__ jobs, const TrkIntr cam,
                                                            const double *__restrict__ world, double *__restrict__ pred)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const MatchPredJob &j = jobs[segment_of([=](int k) { return jobs[k].first; }, n_jobs, i)];
    match_predict(cam, j.R, j.t, world + 3 * (j.src_off + (i - j.first)), pred[2 * i], pred[2 * i + 1]);
}

// row of accumulator register i in lane half h (the C/D map of the 32x32 shapes)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

template <bool ROWS_LO>
__device__ __forceinline__ void gate_tile(v16i &acc, const MatchLine (&P)[16], const double *E, double cx, double cy, double tau2)
{
    if (ROWS_LO) {
        const double n_hi = match_norm_hi(E, cx, cy);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (!match_gate(P[i], cx, cy, n_hi, tau2)) acc[i] = MATCH_NONE;
    } else {
        const MatchLine lo = match_line_lo(E, cx, cy);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (!match_gate(lo, P[i].l0, P[i].l1, P[i].n, tau2)) acc[i] = MATCH_NONE;
    }
}

// tiles [n_tiles] = (task, first row); best, s1, s2 [rows of all tasks]; tau2: the gate's squared bound (rho^2 under the depth gate);
// uv, pred: the keypoints' pixels and the grid's predictions (depth gate only)
template <int MODE>
__global__ __launch_bounds__(SCAN_BLOCK) void match_scan_kernel(const MatchTask *__restrict__ tasks, const int2 *__restrict__ tiles,
                                                                const uint8_t *__restrict__ desc, const int32_t *__restrict__ bias,
                                                                const double *__restrict__ xy, double tau2, int32_t *__restrict__ best,
                                                                int32_t *__restrict__ s1, int32_t *__restrict__ s2,
                                                                const float *__restrict__ uv, const double *__restrict__ pred)
{
    constexpr bool GUIDED = MODE == MATCH_EPIPOLAR;
    const int2 tl = tiles[blockIdx.x];
    const MatchTask &t = tasks[tl.x];
    const int lane = threadIdx.x & 63, cl = lane & 31, h = lane >> 5;
    const int n_a = t.n_a, n_b = t.n_b;
    const int row0 = tl.y + 32 * (threadIdx.x >> 6);
    if (row0 >= n_a) return; // the whole wavefront; nothing below synchronises the workgroup
    v4i A[4];
    {
        const int r = min(row0 + cl, n_a - 1);
        const v4i *p = reinterpret_cast<const v4i *>(desc + (t.a_off + r) * MATCH_DIM + 64 * h);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) A[ks] = p[ks];
    }
    MatchLine P[GUIDED ? 16 : 1];
    double E[9];
    const bool rows_lo = t.rows_lo != 0;
    if constexpr (GUIDED) {
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = t.E[k];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = min(row0 + acc_row(i, h), n_a - 1);
            const double x = xy[2 * (t.a_off + r)], y = xy[2 * (t.a_off + r) + 1];
            if (rows_lo) P[i] = match_line_lo(E, x, y);
            else { MatchLine m; m.l0 = x; m.l1 = y; m.l2 = 0.0; m.n = match_norm_hi(E, x, y); P[i] = m; }
        }
    }
    MatchReproj Q[MODE == MATCH_DEPTH ? 16 : 1];
    if constexpr (MODE == MATCH_DEPTH) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = min(row0 + acc_row(i, h), n_a - 1);
            Q[i].u = (double)uv[2 * (t.a_off + r)]; Q[i].v = (double)uv[2 * (t.a_off + r) + 1];
            Q[i].pu = pred[2 * (t.pred.rows + r)]; Q[i].pv = pred[2 * (t.pred.rows + r) + 1];
        }
    }
    MatchTop top[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) top[i] = match_top_none();

    // the next tile's fragments are asked for before the current tile's products and epilogue, which hide the load
    v4i Bn[4] = {};
    int32_t bn = 0;
    if (n_b > 0) {
        const int64_t cb = t.b_off + min(cl, n_b - 1);
        const v4i *p = reinterpret_cast<const v4i *>(desc + cb * MATCH_DIM + 64 * h);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) Bn[ks] = p[ks];
        bn = bias[cb];
    }
    for (int c0 = 0; c0 < n_b; c0 += 32) {
        const int col = c0 + cl;
        const int64_t cb = t.b_off + min(col, n_b - 1);
        v4i B[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) B[ks] = Bn[ks];
        const int32_t bc = bn;
        if (c0 + 32 < n_b) {
            const int64_t cn = t.b_off + min(col + 32, n_b - 1);
            const v4i *p = reinterpret_cast<const v4i *>(desc + cn * MATCH_DIM + 64 * h);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) Bn[ks] = p[ks];
            bn = bias[cn];
        }
        v16i acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = bc;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[ks], B[ks], acc, 0, 0, 0);
        if constexpr (GUIDED) {
            const double cx = xy[2 * cb], cy = xy[2 * cb + 1];
            if (rows_lo) gate_tile<true>(acc, P, E, cx, cy, tau2);
            else gate_tile<false>(acc, P, E, cx, cy, tau2);
        }
        if constexpr (MODE == MATCH_DEPTH) {
            const int64_t pc = t.pred.cols + min(col, n_b - 1);
            MatchReproj c;
            c.u = (double)uv[2 * cb]; c.v = (double)uv[2 * cb + 1]; c.pu = pred[2 * pc]; c.pv = pred[2 * pc + 1];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (!match_depth_gate(Q[i], c, tau2)) acc[i] = MATCH_NONE;
        }
        if (c0 + 32 > n_b) { // the last, partial tile: the clamped columns are nobody's
            const bool live = col < n_b;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = live ? acc[i] : MATCH_NONE;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) match_top_update(top[i], acc[i], col);
    }
    // once: the 32 lanes of a half hold the same 16 rows (xor butterflies stay inside the half, which wave_ops.h' whole-wave folds
    // do not)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            MatchTop o;
            o.s1 = __shfl_xor(top[i].s1, m, 64); o.best = __shfl_xor(top[i].best, m, 64); o.s2 = __shfl_xor(top[i].s2, m, 64);
            top[i] = match_top_merge(top[i], o);
        }
    }
    if (cl != 0) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = row0 + acc_row(i, h);
        if (r >= n_a) continue;
        const int32_t rc = bias[t.a_off + r] + MATCH_BIAS_CONST;
        const int64_t o = t.out_off + r;
        best[o] = top[i].best;
        s1[o] = top[i].best >= 0 ? top[i].s1 + rc : 0;
        s2[o] = top[i].s2 != MATCH_NONE ? top[i].s2 + rc : 0;
    }
}

struct MatchPairOut { int64_t fwd, rev; }; // first result row of (a, b) and of (b, a)

// flag [n_rows + 1] (the last is 0): forward row i of the chunk is a match
__global__ __launch_bounds__(256) void match_decide_kernel(int64_t n_rows, int n_pairs, const int64_t *__restrict__ row_off,
                                                           const MatchPairOut *__restrict__ po, const int32_t *__restrict__ best,
                                                           const int32_t *__restrict__ s1, const int32_t *__restrict__ s2,
                                                           double max_distance, double max_ratio, int mutual, uint32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n_rows) return;
    if (i == n_rows) { flag[i] = 0; return; }
    const int lo = segment_of(row_off, n_pairs, i);
    const int64_t r = i - row_off[lo], f = po[lo].fwd + r;
    const int32_t c = best[f];
    bool ok = match_accept(c, s1[f], s2[f], max_distance, max_ratio);
    if (ok && mutual) ok = best[po[lo].rev + c] == (int32_t)r;
    flag[i] = ok ? 1u : 0u;
}

// matches / scores [n_out] from position `base` of the whole list on; off [n_pairs] the chunk's part of match_off
__global__ __launch_bounds__(256) void match_write_kernel(int64_t n_rows, int n_pairs, const int64_t *__restrict__ row_off,
                                                          const MatchPairOut *__restrict__ po, const int32_t *__restrict__ best,
                                                          const int32_t *__restrict__ s1, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ excl, int64_t base, int64_t n_out,
                                                          int32_t *__restrict__ matches, int32_t *__restrict__ scores, int64_t *__restrict__ off)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pairs) off[i] = base + excl[row_off[i]];
    if (i >= n_rows || !flag[i]) return;
    const int64_t pos = excl[i];
    if (pos >= n_out) return;
    const int lo = segment_of(row_off, n_pairs, i);
    const int64_t r = i - row_off[lo], f = po[lo].fwd + r;
    matches[2 * pos] = (int32_t)r; matches[2 * pos + 1] = best[f];
    scores[pos] = s1[f];
}

int32_t check_opts(const lvba_match_opts *opts, lvba_match_opts &o)
{
    lvba_match_default_opts(&o);
    if (opts) o = *opts;
    const bool ok = std::isfinite(o.max_distance) && o.max_distance > 0.0 && std::isfinite(o.max_ratio) && o.max_ratio > 0.0 &&
                    o.max_ratio <= 1.0 && (o.mutual == 0 || o.mutual == 1) && o.guided >= MATCH_UNGUIDED && o.guided <= MATCH_DEPTH &&
                    std::isfinite(o.max_epipolar_px) && o.max_epipolar_px > 0.0 && std::isfinite(o.max_reproj_px) && o.max_reproj_px > 0.0;
    if (!ok)
        return lvba_fail(LVBA_ERR_ARG, "options: max_distance %g (finite, > 0), max_ratio %g (in (0, 1]), mutual %d (0 or 1), guided %d (0, 1 "
                         "or 2), max_epipolar_px %g (finite, > 0), max_reproj_px %g (finite, > 0)", o.max_distance, o.max_ratio, o.mutual,
                         o.guided, o.max_epipolar_px, o.max_reproj_px);
    return LVBA_OK;
}

int32_t check_pair(const lvba_match_s *m, int64_t a, int64_t b, const lvba_match_opts &o)
{
    TRY(check_image_pair(a, b, m->kp.n_images));
    if (o.guided == MATCH_DEPTH && !m->has_points)
        return lvba_fail(LVBA_ERR_ARG, "depth-guided matching (guided = 2) needs lvba_match_set_geometry and then lvba_match_set_depth first");
    if (o.guided && !m->has_geometry) return lvba_fail(LVBA_ERR_ARG, "guided matching needs lvba_match_set_geometry first");
    return LVBA_OK;
}

// pred_rows / pred_cols: depth gate only, where the predictions of a's keypoints in b and of b's in a stand (predict_jobs)
MatchTask make_task(const lvba_match_s *m, int a, int b, int64_t out_off, int guided, int64_t pred_rows = 0, int64_t pred_cols = 0)
{
    MatchTask t{};
    t.a_off = m->kp.off[a]; t.b_off = m->kp.off[b]; t.out_off = out_off;
    t.n_a = (int32_t)(m->kp.off[a + 1] - m->kp.off[a]); t.n_b = (int32_t)(m->kp.off[b + 1] - m->kp.off[b]);
    t.rows_lo = a < b ? 1 : 0;
    if (guided == MATCH_EPIPOLAR) {
        const int lo = std::min(a, b), hi = std::max(a, b);
        match_essential(&m->R[9 * (size_t)lo], &m->t[3 * (size_t)lo], &m->R[9 * (size_t)hi], &m->t[3 * (size_t)hi], t.E);
    } else if (guided == MATCH_DEPTH) {
        t.pred.rows = pred_rows; t.pred.cols = pred_cols;
    }
    return t;
}

// The prediction jobs of the unordered pair {a, b}, both orientations: a's keypoints in b at `first`, b's in a behind them.
// Returns the position behind both.
int64_t predict_jobs(const lvba_match_s *m, int a, int b, int64_t first, std::vector<MatchPredJob> &jobs)
{
    const int src[2] = {a, b}, dst[2] = {b, a};
    for (int k = 0; k < 2; ++k) {
        const int64_t n = m->kp.off[src[k] + 1] - m->kp.off[src[k]];
        if (n == 0) continue;
        MatchPredJob j{};
        j.src_off = m->kp.off[src[k]]; j.first = first;
        std::copy_n(&m->R[9 * (size_t)dst[k]], 9, j.R); std::copy_n(&m->t[3 * (size_t)dst[k]], 3, j.t);
        jobs.push_back(j);
        first += n;
    }
    return first;
}

// the scan of `tasks` (results at their out_off in d_best / d_s1 / d_s2), one grid; under the depth gate after the predictions of
// `jobs` (n_pred in all), which the tasks refer to
int32_t scan_tasks(hipStream_t s, const lvba_match_s *m, const std::vector<MatchTask> &tasks, const std::vector<MatchPredJob> &jobs,
                   int64_t n_pred, const lvba_match_opts &o, int32_t *d_best, int32_t *d_s1, int32_t *d_s2)
{
    std::vector<int2> tiles;
    for (size_t k = 0; k < tasks.size(); ++k)
        for (int r = 0; r < tasks[k].n_a; r += SCAN_ROWS) tiles.push_back(make_int2((int)k, r));
    if (tiles.empty()) return LVBA_OK;
    DevArr<MatchTask> d_tasks(s); DevArr<int2> d_tiles(s);
    HIPCHK(d_tasks.alloc_upload(tasks)); HIPCHK(d_tiles.alloc_upload(tiles));
    DevArr<MatchPredJob> d_jobs(s); DevArr<double> d_pred(s);
    if (o.guided == MATCH_DEPTH) {
        HIPCHK(d_pred.alloc(2 * (size_t)n_pred));
        if (n_pred > 0) {
            HIPCHK(d_jobs.alloc_upload(jobs));
            match_predict_kernel<<<grid_for(n_pred, 256), 256, 0, s>>>(n_pred, (int)jobs.size(), d_jobs, m->cam, m->d_pts,
                                                                     d_pred);
            HIPCHK(hipGetLastError());
        }
        match_scan_kernel<MATCH_DEPTH><<<(unsigned)tiles.size(), SCAN_BLOCK, 0, s>>>(d_tasks, d_tiles, m->d_desc,
                                                                                   m->d_bias, nullptr, o.max_reproj_px * o.max_reproj_px, d_best,
                                                                                   d_s1, d_s2, m->kp.d_uv, d_pred);
    } else if (o.guided == MATCH_EPIPOLAR)
        match_scan_kernel<MATCH_EPIPOLAR><<<(unsigned)tiles.size(), SCAN_BLOCK, 0, s>>>(d_tasks, d_tiles, m->d_desc,
                                                                                      m->d_bias, m->kp.d_xy, match_tau2(m->focal_sum, o.max_epipolar_px), d_best, d_s1, d_s2,
                                                                                      nullptr, nullptr);
    else
        match_scan_kernel<MATCH_UNGUIDED><<<(unsigned)tiles.size(), SCAN_BLOCK, 0, s>>>(d_tasks, d_tiles, m->d_desc,
                                                                                      m->d_bias, nullptr, 0.0, d_best, d_s1, d_s2, nullptr,
                                                                                      nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s)); // the task and tile lists go with this scope
    return LVBA_OK;
}

void drop_points(lvba_match_s *m)
{
    if (m->d_pts) {
        (void)hipDeviceSynchronize();
        DevicePool::get().free(m->d_pts);
    }
    m->d_pts = nullptr;
    m->has_points = false;
}

} // namespace

extern "C" void lvba_match_default_opts(lvba_match_opts *o)
{
    if (!o) return;
    *o = lvba_match_opts{};
    o->max_distance = 0.7; o->max_ratio = 0.8; o->mutual = 1; o->guided = 0; o->max_epipolar_px = 4.0; o->max_reproj_px = 8.0;
}

extern "C" int32_t lvba_match_create(int32_t device, int32_t n_images, const int64_t *desc_off, const uint8_t *desc, lvba_match_t *out)
{
    if (!out || n_images < 0 || !desc_off) return lvba_fail(LVBA_ERR_ARG, "null argument or n_images < 0");
    TRY(check_offsets("desc_off", "image", n_images, desc_off, MATCH_MAX_PER_IMAGE));
    const int64_t total = desc_off[n_images];
    if (total > 0 && !desc) return lvba_fail(LVBA_ERR_ARG, "null descriptors");
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_match_s *m = new lvba_match_s;
    m->kp = ImageSet{device, n_images, std::vector<int64_t>(desc_off, desc_off + n_images + 1)};
    if (total > 0) {
        std::vector<uint8_t> biased((size_t)total * MATCH_DIM);
        std::vector<int32_t> bias((size_t)total);
        for (int64_t i = 0; i < total; ++i) {
            int32_t sum = 0;
            for (int k = 0; k < MATCH_DIM; ++k) {
                const uint8_t v = desc[i * MATCH_DIM + k];
                biased[(size_t)i * MATCH_DIM + k] = v ^ 0x80;
                sum += (int32_t)v - 128;
            }
            bias[(size_t)i] = 128 * sum;
        }
        hipError_t e = pool_alloc(&m->d_desc, biased.size());
        if (e == hipSuccess) e = pool_alloc(&m->d_bias, bias.size());
        if (e == hipSuccess) e = lvba::copy_h2d(m->d_desc, biased.data(), biased.size());
        if (e == hipSuccess) e = lvba::copy_h2d(m->d_bias, bias.data(), 4 * bias.size());
        if (e != hipSuccess) {
            lvba_match_destroy(m);
            return lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "descriptor upload: %s", hipGetErrorString(e));
        }
    }
    *out = m;
    return LVBA_OK;
}

extern "C" int32_t lvba_match_destroy(lvba_match_t m)
{
    if (!m) return LVBA_OK;
    (void)hipSetDevice(m->kp.device);
    (void)hipDeviceSynchronize();
    if (m->d_desc) DevicePool::get().free(m->d_desc);
    if (m->d_bias) DevicePool::get().free(m->d_bias);
    image_set_free(m->kp);
    if (m->d_pts) DevicePool::get().free(m->d_pts);
    delete m;
    return LVBA_OK;
}

extern "C" int32_t lvba_match_set_geometry(lvba_match_t m, const float *keypoints_uv, const double *intr, const double *Rcw, const double *tcw)
{
    if (!m || !intr || (m->kp.n_images > 0 && (!Rcw || !tcw))) return lvba_fail(LVBA_ERR_ARG, "null argument");
    const int64_t total = m->kp.off[m->kp.n_images];
    if (total > 0 && !keypoints_uv) return lvba_fail(LVBA_ERR_ARG, "null keypoints");
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    for (int i = 0; i < m->kp.n_images; ++i) {
        const double *R = Rcw + 9 * (size_t)i;
        TRY(check_rotations_finite(Rcw, i, 1));
        TRY(check_translations_finite(tcw, i, 1));
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double d = R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1] + R[3 * a + 2] * R[3 * b + 2] - (a == b ? 1.0 : 0.0);
                if (!(std::fabs(d) <= 1e-6)) return lvba_fail(LVBA_ERR_ARG, "camera %d: rotation not orthonormal within 1e-6", i);
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det > 0.0)) return lvba_fail(LVBA_ERR_ARG, "camera %d: rotation with determinant %g", i, det);
    }
    HIPCHK(hipSetDevice(m->kp.device));
    TRY(image_set_undistort(m->kp, trk_intr_of(intr), keypoints_uv, true));
    drop_points(m); // they were lifted with the poses these replace
    m->cam = trk_intr_of(intr);
    m->R.assign(Rcw, Rcw + 9 * (size_t)m->kp.n_images);
    m->t.assign(tcw, tcw + 3 * (size_t)m->kp.n_images);
    m->focal_sum = intr[0] + intr[1];
    m->has_geometry = true;
    return LVBA_OK;
}

extern "C" int32_t lvba_match_scan(lvba_match_t m, int32_t a, int32_t b, const lvba_match_opts *opts, int32_t *best, int32_t *s1, int32_t *s2)
{
    if (!m) return lvba_fail(LVBA_ERR_ARG, "null handle");
    lvba_match_opts o;
    TRY(check_opts(opts, o));
    TRY(check_pair(m, a, b, o));
    const size_t n_a = (size_t)(m->kp.off[a + 1] - m->kp.off[a]);
    if (n_a > 0 && (!best || !s1 || !s2)) return lvba_fail(LVBA_ERR_ARG, "null output");
    if (n_a == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(m->kp.device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<int32_t> d_out(sg.s);
    HIPCHK(d_out.alloc(3 * n_a));
    int32_t *d = d_out;
    std::vector<MatchPredJob> jobs;
    const int64_t n_pred = o.guided == MATCH_DEPTH ? predict_jobs(m, a, b, 0, jobs) : 0;
    std::vector<MatchTask> tasks{make_task(m, a, b, 0, o.guided, 0, (int64_t)n_a)};
    TRY(scan_tasks(sg.s, m, tasks, jobs, n_pred, o, d, d + n_a, d + 2 * n_a));
    HIPCHK(lvba::copy_d2h(best, d, 4 * n_a));
    HIPCHK(lvba::copy_d2h(s1, d + n_a, 4 * n_a));
    HIPCHK(lvba::copy_d2h(s2, d + 2 * n_a, 4 * n_a));
    return LVBA_OK;
}

extern "C" int32_t lvba_match_pairs(lvba_match_t m, int64_t n_pairs, const int32_t *pairs, const lvba_match_opts *opts, int64_t capacity,
                                    int32_t *matches, int32_t *scores, int64_t *match_off, int64_t *count)
{
    if (!m || !count || !match_off || n_pairs < 0 || capacity < 0 || (n_pairs > 0 && !pairs) || (capacity > 0 && !matches))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_pairs < 0 or capacity < 0");
    lvba_match_opts o;
    TRY(check_opts(opts, o));
    for (int64_t p = 0; p < n_pairs; ++p) TRY(check_pair(m, pairs[2 * p], pairs[2 * p + 1], o));
    *count = 0;
    match_off[0] = 0;
    if (n_pairs == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(m->kp.device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    hipStream_t s = sg.s;
    int64_t base = 0; // matches before the current chunk
    for (int64_t p0 = 0; p0 < n_pairs;) {
        // a chunk: as many pairs as keep the scanned rows of one grid under CHUNK_ROWS (a single pair may exceed it)
        std::vector<MatchTask> tasks;
        std::vector<int64_t> row_off;
        std::vector<MatchPairOut> po;
        std::vector<MatchPredJob> jobs;
        int64_t rows = 0, fwd_rows = 0, n_pred = 0, p1 = p0;
        for (; p1 < n_pairs && p1 - p0 < INT32_MAX / 4; ++p1) {
            const int a = pairs[2 * p1], b = pairs[2 * p1 + 1];
            const int64_t n_a = m->kp.off[a + 1] - m->kp.off[a], n_b = m->kp.off[b + 1] - m->kp.off[b];
            const int64_t need = n_a + (o.mutual ? n_b : 0);
            if (p1 > p0 && rows + need > CHUNK_ROWS) break;
            // the depth gate's predictions cover both images of a pair whatever `mutual` is: they bound the chunk as well
            if (p1 > p0 && o.guided == MATCH_DEPTH && n_pred + n_a + n_b > CHUNK_ROWS) break;
            MatchPairOut q; q.fwd = rows; q.rev = rows + n_a;
            const int64_t pa = n_pred, pb = n_pred + n_a; // a's keypoints in b, b's in a
            if (o.guided == MATCH_DEPTH) n_pred = predict_jobs(m, a, b, n_pred, jobs);
            tasks.push_back(make_task(m, a, b, q.fwd, o.guided, pa, pb));
            if (o.mutual) tasks.push_back(make_task(m, b, a, q.rev, o.guided, pb, pa));
            row_off.push_back(fwd_rows); po.push_back(q);
            rows += need; fwd_rows += n_a;
        }
        const int np = (int)(p1 - p0);
        row_off.push_back(fwd_rows);
        if (fwd_rows > 0) {
            DevArr<int32_t> d_res(s); DevArr<int64_t> d_row_off(s); DevArr<MatchPairOut> d_po(s);
            DevArr<uint32_t> d_flag(s), d_excl(s); DevArr<int64_t> d_off(s); DevArr<int32_t> d_m(s), d_sc(s);
            HIPCHK(d_res.alloc(3 * (size_t)rows));
            int32_t *d_best = d_res, *d_s1 = d_best + rows, *d_s2 = d_s1 + rows;
            TRY(scan_tasks(s, m, tasks, jobs, n_pred, o, d_best, d_s1, d_s2));
            HIPCHK(d_flag.alloc((size_t)fwd_rows + 1)); HIPCHK(d_excl.alloc((size_t)fwd_rows + 1)); HIPCHK(d_off.alloc((size_t)np));
            HIPCHK(d_row_off.alloc_upload(row_off)); HIPCHK(d_po.alloc_upload(po));
            match_decide_kernel<<<grid_for(fwd_rows + 1, 256), 256, 0, s>>>(fwd_rows, np, d_row_off, d_po, d_best,
                                                                          d_s1, d_s2, o.max_distance, o.max_ratio, o.mutual, d_flag);
            HIPCHK(hipGetLastError());
            TRY(scan_excl<uint32_t>(s, d_flag, d_excl, (size_t)fwd_rows + 1));
            uint32_t found = 0;
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(copy_d2h(&found, d_excl + fwd_rows, d_excl.bytes(1)));
            const int64_t n_out = std::max<int64_t>(0, std::min<int64_t>(found, capacity - base));
            HIPCHK(d_m.alloc(2 * (size_t)n_out)); HIPCHK(d_sc.alloc((size_t)n_out));
            match_write_kernel<<<grid_for(std::max<int64_t>(fwd_rows, np), 256), 256, 0, s>>>(
                fwd_rows, np, d_row_off, d_po, d_best, d_s1, d_flag, d_excl, base,
                n_out, d_m, d_sc, d_off);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(d_off.download(match_off + p0, (size_t)np));
            if (n_out > 0) {
                HIPCHK(d_m.download(matches + 2 * base, 2 * (size_t)n_out));
                if (scores) HIPCHK(d_sc.download(scores + base, (size_t)n_out));
            }
            base += found;
        } else {
            for (int64_t p = p0; p < p1; ++p) match_off[p] = base;
        }
        p0 = p1;
    }
    match_off[n_pairs] = base;
    *count = base;
    return LVBA_OK;
}

extern "C" int32_t lvba_match_set_depth(lvba_match_t m, lvba_depth_t depth)
{
    if (!m) return lvba_fail(LVBA_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->kp.device));
    if (!depth) {
        drop_points(m);
        return LVBA_OK;
    }
    if (!m->has_geometry) return lvba_fail(LVBA_ERR_ARG, "lvba_match_set_depth needs lvba_match_set_geometry first");
    if (depth->n_images != m->kp.n_images)
        return lvba_fail(LVBA_ERR_ARG, "the depth set holds %d images, the matcher %d", depth->n_images, m->kp.n_images);
    if (depth->device != m->kp.device)
        return lvba_fail(LVBA_ERR_ARG, "the depth set lives on device %d, the matcher on device %d", depth->device, m->kp.device);
    const int64_t total = m->kp.off[m->kp.n_images];
    if (total > 0) {
        ScopedStream sg;
        HIPCHK(sg.acquire());
        DevArr<double> d_new(sg.s), d_R(sg.s), d_t(sg.s); // the old table stays until the new one stands
        HIPCHK(d_new.alloc(3 * (size_t)total));
        TRY(image_set_upload(m->kp, true, nullptr)); // the offsets go up with the first lift and stay
        HIPCHK(d_R.alloc_upload(m->R)); HIPCHK(d_t.alloc_upload(m->t));
        match_lift_kernel<<<grid_for(total, 256), 256, 0, sg.s>>>(total, m->kp.n_images, m->kp.d_off, m->kp.d_uv, m->kp.d_xy, depth->d_depth,
                                                                depth->width, depth->height, d_R, d_t,
                                                                d_new);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(sg.s));
        drop_points(m);
        m->d_pts = (double *)d_new.release();
    }
    m->has_points = true;
    return LVBA_OK;
}

extern "C" int32_t lvba_match_points(lvba_match_t m, double *world)
{
    if (!m) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (!m->has_points) return lvba_fail(LVBA_ERR_ARG, "no lifted points: lvba_match_set_depth first");
    const int64_t total = m->kp.off[m->kp.n_images];
    if (total == 0) return LVBA_OK;
    if (!world) return lvba_fail(LVBA_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(m->kp.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(lvba::copy_d2h(world, m->d_pts, 24 * (size_t)total));
    return LVBA_OK;
}
