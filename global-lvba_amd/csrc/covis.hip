// covis.hip -- which image pairs to match, from LiDAR co-visibility: a grid of samples per image lifted through the image's own
// depth image, projected into every other image and tested against that image's depth for occlusion (lvba_covis_*; the rule is
// in include/lvba_hip.h, its scalar pieces in covis_device.h).
//
// Device design:
//   covis_lift_kernel    a thread per cell: the first pixel of the ring search with a depth return -> the resident [M][G][3] fp64
//                        table, NaN rows where a cell has no point.  Inside every call: the table is 4.6 KB per image.
//   covis_count_kernel   the hot one, M^2 G projections and fetches.  A wavefront owns one (source i, target j) and walks i's
//                        samples 64 at a time; pose j and the intrinsics are uniform (scalar registers), the count is
//                        popcount(ballot(seen)) in a scalar, lane 0 stores counts[i][j].  The four wavefronts of a workgroup hold
//                        four sources for the SAME target, and the grid is target-major, so that depth image j -- the only
//                        scattered read -- is shared by workgroups that run close in time (all eight XCDs on the same image at
//                        once; DESIGN.md §10i has what a contiguous part of the order per XCD gave instead).  The wavefront on
//                        the diagonal counts the samples that have a point instead: n_points[i].
//   covis_select_kernel  cap only: a wavefront per image, K arg-max rounds over its row of scores; each round takes the best
//                        partner behind the previous round's, so nothing is marked.  Result: the image's K-th best partner.
//   covis_flag_kernel    a wavefront per image i: how many pairs (i, j > i) are kept; then an exclusive prefix sum of the M numbers,
//   covis_write_kernel   and the same walk again writes the pairs in (i, j) order at their positions.
// No atomics of any kind and no LDS: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "image_set.h"
#include "covis_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int COVIS_BLOCK = 256;                 // four wavefronts
constexpr int COVIS_WAVES = COVIS_BLOCK / 64;    // sources per workgroup of the count kernel, images per workgroup elsewhere

struct CovisShape { int32_t M, W, H, grid_x, grid_y, G, radius; };

__global__ __launch_bounds__(COVIS_BLOCK) void covis_lift_kernel(const CovisShape sh, const float *__restrict__ depth,
                                                                 const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                                 const TrkIntr cam, double *__restrict__ world)
{
    const int64_t idx = (int64_t)blockIdx.x * COVIS_BLOCK + threadIdx.x;
    if (idx >= (int64_t)sh.M * sh.G) return;
    const int m = (int)(idx / sh.G), s = (int)(idx % sh.G);
    const int gx = s % sh.grid_x, gy = s / sh.grid_x;
    covis_sample(depth + (int64_t)m * sh.W * sh.H, sh.W, sh.H, cam, covis_centre(gx, sh.grid_x, sh.W), covis_centre(gy, sh.grid_y, sh.H),
                 sh.radius, Rcw + 9 * (int64_t)m, tcw + 3 * (int64_t)m, world + 3 * idx);
}

// groups = ceil(M / 4) workgroups per target; the grid has M groups workgroups, target-major
__global__ __launch_bounds__(COVIS_BLOCK) void covis_count_kernel(const CovisShape sh, int groups,
                                                                  const double *__restrict__ world, const float *__restrict__ depth,
                                                                  const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                                  const TrkIntr cam, const CovisRule o, int32_t *__restrict__ n_points,
                                                                  int32_t *__restrict__ counts)
{
    const int j = (int)(blockIdx.x / (unsigned)groups);
    const int i = (int)(blockIdx.x % (unsigned)groups) * COVIS_WAVES + (int)(threadIdx.x >> 6);
    if (i >= sh.M) return; // the whole wavefront; nothing below synchronises the workgroup
    const int lane = threadIdx.x & 63;
    const double *__restrict__ Rj = Rcw + 9 * (int64_t)j, *__restrict__ tj = tcw + 3 * (int64_t)j;
    const float *__restrict__ dj = depth + (int64_t)j * sh.W * sh.H;
    const double *__restrict__ Xi = world + 3 * (int64_t)i * sh.G;
    int32_t total = 0;
    for (int s0 = 0; s0 < sh.G; s0 += 64) {
        const int s = s0 + lane;
        double X[3] = {NAN, NAN, NAN};
        if (s < sh.G) { X[0] = Xi[3 * s]; X[1] = Xi[3 * s + 1]; X[2] = Xi[3 * s + 2]; }
        const bool hit = i == j ? X[0] == X[0] : covis_seen(cam, dj, sh.W, sh.H, Rj, tj, X, o);
        total += (int32_t)__popcll(__ballot(hit));
    }
    if (lane != 0) return;
    if (i == j) n_points[i] = total;
    counts[(int64_t)i * sh.M + j] = i == j ? 0 : total;
}

__device__ __forceinline__ CovisPair pair_of(int M, int i, int j, const int32_t *__restrict__ n_points, const int32_t *__restrict__ counts,
                                             const CovisRule &o)
{
    return covis_pair(counts[(int64_t)i * M + j], counts[(int64_t)j * M + i], n_points[i], n_points[j], o);
}

// kth [M]: the K-th best eligible partner of every image, the last place where it has fewer than K
__global__ __launch_bounds__(COVIS_BLOCK) void covis_select_kernel(int M, int K, const int32_t *__restrict__ n_points,
                                                                   const int32_t *__restrict__ counts, const CovisRule o,
                                                                   CovisRank *__restrict__ kth)
{
    const int i = blockIdx.x * COVIS_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;
    CovisRank prev = covis_rank_first();
    for (int k = 0; k < K; ++k) {
        CovisRank best = covis_rank_last();
        for (int p = lane; p < M; p += 64) {
            if (p == i) continue;
            const CovisPair pr = pair_of(M, i, p, n_points, counts, o);
            CovisRank c; c.score = pr.score; c.partner = p;
            if (pr.eligible && covis_rank_before(prev, c) && covis_rank_before(c, best)) best = c;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) { // the order is total: every lane ends with the same place
            CovisRank other; other.score = __shfl_xor(best.score, m, 64); other.partner = __shfl_xor(best.partner, m, 64);
            if (covis_rank_before(other, best)) best = other;
        }
        prev = best;
        if (best.partner == INT32_MAX) break; // fewer than K eligible partners: all of them are within the cap
    }
    if (lane == 0) kth[i] = prev;
}

// kth = nullptr: no cap
__device__ __forceinline__ bool pair_kept(int M, int i, int j, const int32_t *__restrict__ n_points, const int32_t *__restrict__ counts,
                                          const CovisRule &o, const CovisRank *__restrict__ kth, CovisPair &pr)
{
    pr = pair_of(M, i, j, n_points, counts, o);
    if (!pr.eligible) return false;
    return !kth || covis_within_cap(pr.score, j, kth[i]) || covis_within_cap(pr.score, i, kth[j]);
}

// row_count [M + 1] (the last is 0): the kept pairs (i, j > i) of image i
__global__ __launch_bounds__(COVIS_BLOCK) void covis_flag_kernel(int M, const int32_t *__restrict__ n_points, const int32_t *__restrict__ counts,
                                                                 const CovisRule o, const CovisRank *__restrict__ kth,
                                                                 uint32_t *__restrict__ row_count)
{
    const int i = blockIdx.x * COVIS_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i > M) return;
    uint32_t total = 0;
    for (int j0 = i + 1; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        CovisPair pr;
        const bool keep = j < M && pair_kept(M, i, j, n_points, counts, o, kth, pr);
        total += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) row_count[i] = total;
}

// pairs [n_out][2], score [n_out], shared [n_out][2] = (c_ij, c_ji): the kept pairs by (i, j), those with a position below n_out
__global__ __launch_bounds__(COVIS_BLOCK) void covis_write_kernel(int M, const int32_t *__restrict__ n_points, const int32_t *__restrict__ counts,
                                                                  const CovisRule o, const CovisRank *__restrict__ kth,
                                                                  const uint32_t *__restrict__ row_first, int64_t n_out,
                                                                  int32_t *__restrict__ pairs, double *__restrict__ score,
                                                                  int32_t *__restrict__ shared)
{
    const int i = blockIdx.x * COVIS_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;
    int64_t first = row_first[i];
    for (int j0 = i + 1; j0 < M && first < n_out; j0 += 64) {
        const int j = j0 + lane;
        CovisPair pr;
        const bool keep = j < M && pair_kept(M, i, j, n_points, counts, o, kth, pr);
        const uint64_t mask = __ballot(keep);
        const int64_t pos = first + __popcll(mask & (((uint64_t)1 << lane) - 1));
        if (keep && pos < n_out) {
            pairs[2 * pos] = i; pairs[2 * pos + 1] = j;
            score[pos] = pr.score;
            shared[2 * pos] = counts[(int64_t)i * M + j]; shared[2 * pos + 1] = counts[(int64_t)j * M + i];
        }
        first += __popcll(mask);
    }
}

struct CovisCall {
    CovisShape sh;
    CovisRule rule;
    TrkIntr cam;
};

int32_t check_call(lvba_depth_t depth, const double *Rcw, const double *tcw, const double *intr, const lvba_covis_opts *opts, CovisCall &c)
{
    if (!depth || !intr) return lvba_fail(LVBA_ERR_ARG, "null depth handle or intrinsics");
    const int M = depth->n_images, W = depth->width, H = depth->height;
    if (M > 0 && (!Rcw || !tcw)) return lvba_fail(LVBA_ERR_ARG, "null poses");
    if (M > COVIS_MAX_IMAGES) // before anything is read of the poses
        return lvba_fail(LVBA_ERR_UNSUPPORTED, "%d images (at most %d: the count matrix is [M][M])", M, COVIS_MAX_IMAGES);
    lvba_covis_opts o;
    lvba_covis_default_opts(&o);
    if (opts) o = *opts;
    const bool ok = o.grid_x >= 1 && o.grid_x <= COVIS_MAX_GRID && o.grid_y >= 1 && o.grid_y <= COVIS_MAX_GRID && o.search_radius >= 0 &&
                    o.search_radius <= COVIS_MAX_RADIUS && (o.occlusion == 0 || o.occlusion == 1) && (o.both_ways == 0 || o.both_ways == 1) &&
                    o.max_per_image >= 0 && o.max_per_image <= COVIS_MAX_PER_IMAGE && o.min_shared >= 0 && std::isfinite(o.min_overlap) &&
                    o.min_overlap >= 0.0 && o.min_overlap <= 1.0 && std::isfinite(o.occlusion_rel) && o.occlusion_rel >= 0.0 &&
                    std::isfinite(o.occlusion_abs) && o.occlusion_abs >= 0.0;
    if (!ok)
        return lvba_fail(LVBA_ERR_ARG, "options: grid %d x %d (1 .. 64 each), search_radius %d (0 .. 16), occlusion %d, both_ways %d (0 or 1), "
                         "max_per_image %d (0 .. 1024), min_shared %d (>= 0), min_overlap %g (in [0, 1]), occlusion_rel %g, occlusion_abs %g "
                         "(finite, >= 0)", o.grid_x, o.grid_y, o.search_radius, o.occlusion, o.both_ways, o.max_per_image, o.min_shared,
                         o.min_overlap, o.occlusion_rel, o.occlusion_abs);
    if (o.grid_x > W - 1 || o.grid_y > H - 1)
        return lvba_fail(LVBA_ERR_ARG, "a grid of %d x %d cells on images of %d x %d (at most width - 1, height - 1)", o.grid_x, o.grid_y, W, H);
    TRY(check_intrinsics_finite(intr));
    TRY(check_rotations_finite(Rcw, 0, M));
    TRY(check_translations_finite(tcw, 0, M));
    c.sh = CovisShape{M, W, H, o.grid_x, o.grid_y, o.grid_x * o.grid_y, o.search_radius};
    c.rule = CovisRule{o.occlusion, o.both_ways, o.max_per_image, o.min_shared, o.min_overlap, o.occlusion_rel, o.occlusion_abs};
    c.cam = trk_intr_of(intr);
    return LVBA_OK;
}

// the device side of a call (M >= 1): the poses and the sample table; with counts, n_points [M] and counts [M][M] behind it
struct CovisWork {
    DevArr<double> R, t, world; DevArr<int32_t> n_points, counts;
    explicit CovisWork(hipStream_t s) : R(s), t(s), world(s), n_points(s), counts(s) {}
};

int32_t run_lift(hipStream_t s, lvba_depth_t depth, const double *Rcw, const double *tcw, const CovisCall &c, CovisWork &w)
{
    const size_t M = (size_t)c.sh.M;
    HIPCHK(w.R.alloc(9 * M)); HIPCHK(w.t.alloc(3 * M)); HIPCHK(w.world.alloc(3 * M * (size_t)c.sh.G));
    HIPCHK(w.R.upload(Rcw, 9 * M)); HIPCHK(w.t.upload(tcw, 3 * M));
    covis_lift_kernel<<<grid_for((int64_t)M * c.sh.G, COVIS_BLOCK), COVIS_BLOCK, 0, s>>>(c.sh, depth->d_depth, w.R, w.t,
                                                                                      c.cam, w.world);
    HIPCHK(hipGetLastError());
    return LVBA_OK;
}

int32_t run_counts(hipStream_t s, lvba_depth_t depth, const double *Rcw, const double *tcw, const CovisCall &c, CovisWork &w)
{
    TRY(run_lift(s, depth, Rcw, tcw, c, w));
    const int M = c.sh.M, groups = (M + COVIS_WAVES - 1) / COVIS_WAVES;
    HIPCHK(w.n_points.alloc((size_t)M)); HIPCHK(w.counts.alloc((size_t)M * M));
    covis_count_kernel<<<(unsigned)((int64_t)M * groups), COVIS_BLOCK, 0, s>>>(c.sh, groups, w.world, depth->d_depth,
                                                                              w.R, w.t, c.cam, c.rule,
                                                                              w.n_points, w.counts);
    HIPCHK(hipGetLastError());
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_covis_default_opts(lvba_covis_opts *o)
{
    if (!o) return;
    *o = lvba_covis_opts{};
    o->grid_x = 16; o->grid_y = 12; o->search_radius = 4; o->occlusion = 1; o->both_ways = 0; o->max_per_image = 0; o->min_shared = 8;
    o->min_overlap = 0.1; o->occlusion_rel = 0.05; o->occlusion_abs = 0.1;
}

extern "C" int32_t lvba_covis_samples(lvba_depth_t depth, const double *Rcw, const double *tcw, const double *intr, const lvba_covis_opts *opts,
                                      double *world)
{
    CovisCall c;
    TRY(check_call(depth, Rcw, tcw, intr, opts, c));
    if (c.sh.M == 0) return LVBA_OK;
    if (!world) return lvba_fail(LVBA_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(depth->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    CovisWork w(sg.s);
    TRY(run_lift(sg.s, depth, Rcw, tcw, c, w));
    HIPCHK(hipStreamSynchronize(sg.s));
    HIPCHK(w.world.download(world, 3 * (size_t)c.sh.M * c.sh.G));
    return LVBA_OK;
}

extern "C" int32_t lvba_covis_counts(lvba_depth_t depth, const double *Rcw, const double *tcw, const double *intr, const lvba_covis_opts *opts,
                                     int32_t *n_points, int32_t *counts)
{
    CovisCall c;
    TRY(check_call(depth, Rcw, tcw, intr, opts, c));
    if (c.sh.M == 0) return LVBA_OK;
    if (!n_points || !counts) return lvba_fail(LVBA_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(depth->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    CovisWork w(sg.s);
    TRY(run_counts(sg.s, depth, Rcw, tcw, c, w));
    HIPCHK(hipStreamSynchronize(sg.s));
    HIPCHK(w.n_points.download(n_points, (size_t)c.sh.M)); HIPCHK(w.counts.download(counts, (size_t)c.sh.M * c.sh.M));
    return LVBA_OK;
}

extern "C" int32_t lvba_covis_pairs(lvba_depth_t depth, const double *Rcw, const double *tcw, const double *intr, const lvba_covis_opts *opts,
                                    int64_t capacity, int32_t *pairs, double *score, int32_t *shared, int64_t *count)
{
    CovisCall c;
    TRY(check_call(depth, Rcw, tcw, intr, opts, c));
    if (!count || capacity < 0 || (capacity > 0 && !pairs)) return lvba_fail(LVBA_ERR_ARG, "null count, capacity < 0, or capacity > 0 without pairs");
    *count = 0;
    const int M = c.sh.M;
    if (M < 2) return LVBA_OK;
    HIPCHK(hipSetDevice(depth->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    hipStream_t s = sg.s;
    CovisWork w(s);
    TRY(run_counts(s, depth, Rcw, tcw, c, w));
    const int32_t *d_n = w.n_points, *d_c = w.counts;
    DevArr<CovisRank> d_kth(s); DevArr<uint32_t> d_row(s), d_first(s); DevArr<int32_t> d_pairs(s); DevArr<double> d_score(s);
    DevArr<int32_t> d_shared(s);
    const CovisRank *kth = nullptr;
    const int K = c.rule.max_per_image;
    if (K > 0 && K < M - 1) { // with K >= M - 1 every partner is within the cap
        HIPCHK(d_kth.alloc((size_t)M));
        covis_select_kernel<<<grid_for(M, COVIS_WAVES), COVIS_BLOCK, 0, s>>>(M, K, d_n, d_c, c.rule, d_kth);
        HIPCHK(hipGetLastError());
        kth = d_kth;
    }
    HIPCHK(d_row.alloc((size_t)M + 1)); HIPCHK(d_first.alloc((size_t)M + 1));
    covis_flag_kernel<<<grid_for(M + 1, COVIS_WAVES), COVIS_BLOCK, 0, s>>>(M, d_n, d_c, c.rule, kth, d_row);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, d_row, d_first, (size_t)M + 1));
    uint32_t found = 0;
    HIPCHK(copy_d2h(&found, d_first + M, d_first.bytes(1)));
    const int64_t n_out = std::min<int64_t>(found, capacity);
    if (n_out > 0) {
        HIPCHK(d_pairs.alloc(2 * (size_t)n_out)); HIPCHK(d_score.alloc((size_t)n_out)); HIPCHK(d_shared.alloc(2 * (size_t)n_out));
        covis_write_kernel<<<grid_for(M, COVIS_WAVES), COVIS_BLOCK, 0, s>>>(M, d_n, d_c, c.rule, kth, d_first, n_out,
                                                                          d_pairs, d_score, d_shared);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(d_pairs.download(pairs, 2 * (size_t)n_out));
        if (score) HIPCHK(d_score.download(score, (size_t)n_out));
        if (shared) HIPCHK(d_shared.download(shared, 2 * (size_t)n_out));
    }
    *count = found;
    return LVBA_OK;
}
