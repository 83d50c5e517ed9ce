// photo.hip -- multi-view colour fusion and photometric consistency of the map (lvba_photo_*; the rule is in include/lvba_hip.h,
// its scalar pieces in photo_device.h, also compiled for the host by the tests).
//
// Device design.  A handle holds the float points and their integer totals (n_views, S1 [3], S2 [3]).  The images of a call come
// in batches sized by the free memory and stay as the bytes that were uploaded (a repack to one word per texel was measured: the
// sample pass was 4 % slower on it); per batch:
//   photo_sample_kernel  the hot path.  A workgroup owns 256 consecutive points; a lane keeps its point, n_views, S1 [3] and
//                        S2 [3] in registers and walks the images of the resident batch in index order.  R_j, t_j and the image
//                        and depth base addresses depend on the loop counter and the kernel arguments alone: workgroup-uniform,
//                        scalar loads.  Most (point, image) pairs end at BEHIND or OUTSIDE after the projection; the survivors
//                        do four depth gathers and four texel gathers of three bytes each.  At the end of the batch the lane
//                        adds its counters to the point's totals -- the point is the lane's alone, the batches follow each
//                        other on one stream: no atomics.
//   photo_finish_kernel  one lane per point: rgb and sigma, and per workgroup the numbers of seen and valid points, of samples,
//                        and the sum of sigma over the valid points (the DPP trees of wave_ops.h, then four values through
//                        LDS); the host adds the workgroups' shares in index order.
// The totals are integers: no floating-point sum crosses lanes before the finish, and nothing depends on the batching.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "image_set.h"
#include "photo_device.h"
#include "expo_device.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

struct lvba_photo_s {
    int device = 0;
    int64_t n = 0;
    int n_images = 0, width = 0, height = 0;
    TrkIntr cam{};
    PhotoRule rule{};
    int32_t max_batch = 0;
    lvba_depth_t depth = nullptr;  // the caller's, kept alive by the caller
    std::vector<uint8_t> added;    // [n_images]
    // handle-owned device arrays (no stream: every call has drained its own before it returned)
    DevArr<float> xyz;             // [n][3]
    DevArr<int32_t> n_views;       // [n]
    DevArr<uint32_t> s1;           // [n][3]
    DevArr<int64_t> s2;            // [n][3]
    double ms[3] = {0, 0, 0};      // upload, sample pass, finish: accumulated
    ~lvba_photo_s()
    {
        (void)hipSetDevice(device);
        xyz.reset(); n_views.reset(); s1.reset(); s2.reset();
    }
};

namespace {

constexpr int PHOTO_BLOCK = 256; // the sample kernel's chunk of points

// images 0 .. B - 1 of the batch: Rcw [B][9], tcw [B][3], bgr [B][H][W][3] as uploaded; depth0 = the depth image of the batch's
// first image (null: no occlusion test).  The counters of point i are added to n_views [i], s1 [i][3], s2 [i][3].  GAINS: the
// exposure compensation (expo_device.h) -- gains [B][3][2] depend on the loop counter alone, scalar loads like the pose, and
// every channel of a sample goes through expo_apply before it is added; the plain instantiation never reads `gains` and is the
// kernel it was (DESIGN.md §10r has the resource figures of both).
template <bool GAINS>
__global__ __launch_bounds__(PHOTO_BLOCK) void photo_sample_kernel(int64_t n, const float *__restrict__ xyz, int B,
                                                                   const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                                                   const uint8_t *__restrict__ bgr, const float *__restrict__ depth0,
                                                                   const TrkIntr cam, const PhotoRule o, int W, int H,
                                                                   int32_t *__restrict__ n_views, uint32_t *__restrict__ s1,
                                                                   int64_t *__restrict__ s2, const int64_t *__restrict__ gains)
{
    const int64_t i = (int64_t)blockIdx.x * PHOTO_BLOCK + threadIdx.x;
    if (i >= n) return; // nothing below synchronises the workgroup
    const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
    const int64_t npix = (int64_t)W * H;
    PhotoSums acc;
    acc.n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc.s1[k] = 0u; acc.s2[k] = 0; }
    for (int b = 0; b < B; ++b) { // uniform
        const uint8_t *__restrict__ tb = bgr + 3 * (int64_t)b * npix;
        const float *__restrict__ db = depth0 ? depth0 + (int64_t)b * npix : nullptr;
        int32_t c16[3];
        if (photo_sample(cam, db, W, H, Rcw + 9 * (int64_t)b, tcw + 3 * (int64_t)b, X, o,
                         [&](int y, int x) { return photo_texel_of(tb + 3 * ((int64_t)y * W + x)); }, c16)) {
            if (GAINS) {
                const int64_t *__restrict__ g = gains + 6 * (int64_t)b;
#pragma unroll
                for (int k = 0; k < 3; ++k) c16[k] = expo_apply(g[2 * k], g[2 * k + 1], c16[k]);
            }
            photo_add(acc, c16);
        }
    }
    if (acc.n == 0) return;
    n_views[i] += acc.n;
#pragma unroll
    for (int k = 0; k < 3; ++k) { s1[3 * i + k] += acc.s1[k]; s2[3 * i + k] += acc.s2[k]; }
}

// rgb [n][3], sigma [n]; part_i [gridDim.x][3] = seen points, valid points, samples of the workgroup; part_s [gridDim.x] = its
// sum of sigma over the valid points
__global__ __launch_bounds__(256) void photo_finish_kernel(int64_t n, const int32_t *__restrict__ n_views, const uint32_t *__restrict__ s1,
                                                           const int64_t *__restrict__ s2, int32_t min_views, uint8_t *__restrict__ rgb,
                                                           double *__restrict__ sigma, int32_t *__restrict__ part_i,
                                                           double *__restrict__ part_s)
{
    __shared__ int32_t red_i[4][3];
    __shared__ double red_s[4];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int seen = 0, valid = 0, samples = 0;
    double sg = 0.0;
    if (i < n) {
        PhotoSums s;
        s.n = n_views[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) { s.s1[k] = s1[3 * i + k]; s.s2[k] = s2[3 * i + k]; }
        uint8_t c[3];
        photo_rgb(s, c);
        rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2];
        const double v = photo_sigma(s, min_views);
        sigma[i] = v;
        seen = s.n >= 1 ? 1 : 0;
        valid = s.n >= min_views ? 1 : 0;
        samples = s.n; // a workgroup's total is at most 256 * 32 768
        if (valid) sg = v;
    }
    seen = wave_fold_to_lane63<SumStepI32>(seen);
    valid = wave_fold_to_lane63<SumStepI32>(valid);
    samples = wave_fold_to_lane63<SumStepI32>(samples);
    sg = wave_sum_to_lane63(sg);
    if ((threadIdx.x & 63) == 63) {
        const int wv = threadIdx.x >> 6;
        red_i[wv][0] = seen; red_i[wv][1] = valid; red_i[wv][2] = samples; red_s[wv] = sg;
    }
    __syncthreads();
    if (threadIdx.x < 3) part_i[3 * (int64_t)blockIdx.x + threadIdx.x] = red_i[0][threadIdx.x] + red_i[1][threadIdx.x] + red_i[2][threadIdx.x] + red_i[3][threadIdx.x];
    if (threadIdx.x == 3) part_s[blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
}

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

} // namespace

extern "C" void lvba_photo_default_opts(lvba_photo_opts *o)
{
    if (!o) return;
    *o = lvba_photo_opts{};
    o->occlusion_rel = 0.05; o->occlusion_abs = 0.1; // the co-visibility stage's
    o->max_depth = 0.0; o->holes = 0; o->min_views = 2; o->max_batch_images = 0; o->reserved = 0;
}

extern "C" int32_t lvba_photo_create(int32_t device, int64_t n, const float *xyz, int32_t n_images, int32_t width, int32_t height,
                                     const double *intr, lvba_depth_t depth, const lvba_photo_opts *opts, lvba_photo_t *out)
{
    if (!out) return lvba_fail(LVBA_ERR_ARG, "null output");
    if (!intr || (n > 0 && !xyz)) return lvba_fail(LVBA_ERR_ARG, "null points or intrinsics");
    if (n < 0 || n >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_ARG, "%lld points (0 .. 2^32 - 1)", (long long)n);
    if (width < 2 || height < 2) return lvba_fail(LVBA_ERR_ARG, "image size %d x %d (both must be >= 2)", width, height);
    if (n_images < 1 || n_images > PHOTO_MAX_IMAGES) return lvba_fail(LVBA_ERR_ARG, "%d images (1 .. %d)", n_images, PHOTO_MAX_IMAGES);
    if (depth && (depth->n_images != n_images || depth->width != width || depth->height != height || depth->device != device))
        return lvba_fail(LVBA_ERR_ARG, "depth set of %d images of %d x %d on device %d; the images are %d of %d x %d on device %d",
                         depth->n_images, depth->width, depth->height, depth->device, n_images, width, height, device);
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    lvba_photo_opts o;
    lvba_photo_default_opts(&o);
    if (opts) o = *opts;
    if (!finite_nonneg(o.occlusion_rel) || !finite_nonneg(o.occlusion_abs) || !finite_nonneg(o.max_depth) || o.min_views < 2 ||
        o.max_batch_images < 0)
        return lvba_fail(LVBA_ERR_ARG, "options: occlusion_rel %g, occlusion_abs %g, max_depth %g (finite, >= 0), min_views %d (>= 2), "
                         "max_batch_images %d (>= 0)", o.occlusion_rel, o.occlusion_abs, o.max_depth, o.min_views, o.max_batch_images);
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_photo_s *h = new (std::nothrow) lvba_photo_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    struct Guard { lvba_photo_s *h; ~Guard() { delete h; } } guard{h};
    h->device = device; h->n = n; h->n_images = n_images; h->width = width; h->height = height;
    h->cam = trk_intr_of(intr);
    h->rule = photo_rule_of(depth != nullptr, o.occlusion_rel, o.occlusion_abs, o.max_depth, o.holes, o.min_views);
    h->max_batch = o.max_batch_images;
    h->depth = depth;
    h->added.assign((size_t)n_images, 0);
    const size_t N = (size_t)n;
    HIPCHK(h->xyz.alloc(3 * N)); HIPCHK(h->n_views.alloc(N)); HIPCHK(h->s1.alloc(3 * N)); HIPCHK(h->s2.alloc(3 * N));
    if (n > 0) {
        HIPCHK(h->xyz.upload(xyz, 3 * N));
        HIPCHK(hipMemset(h->n_views, 0, h->n_views.bytes(N)));
        HIPCHK(hipMemset(h->s1, 0, h->s1.bytes(3 * N)));
        HIPCHK(hipMemset(h->s2, 0, h->s2.bytes(3 * N)));
        HIPCHK(hipDeviceSynchronize());
    }
    *out = h;
    guard.h = nullptr;
    return LVBA_OK;
}

// Both entry points.  gains [n][3][2] or null: the plain kernel.
static int32_t photo_add_images(lvba_photo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                                const int64_t *gains)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (first < 0 || n < 0 || (int64_t)first + n > h->n_images || (n > 0 && first >= h->n_images))
        return lvba_fail(LVBA_ERR_ARG, "images [%d, %d + %d) of %d", first, first, n, h->n_images);
    if (n == 0) return LVBA_OK;
    if (!Rcw || !tcw || !bgr) return lvba_fail(LVBA_ERR_ARG, "null cameras or images");
    TRY(check_rotations_finite(Rcw, 0, n));
    TRY(check_translations_finite(tcw, 0, n));
    for (int k = 0; k < n; ++k)
        if (h->added[(size_t)first + k]) return lvba_fail(LVBA_ERR_ARG, "image %d was added before", first + k);
    if (gains && !expo_gains_ok(gains, 3 * (int64_t)n))
        return lvba_fail(LVBA_ERR_ARG, "gains: A outside [2^14, 2^18] or |B| above 2^16 * 65280");
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)h->width * h->height;
    // the batch: the uploaded bytes of B images
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(0.4 * ((double)free_b + (double)DevicePool::get().cached_bytes()), 8.0 * (1 << 30));
    int64_t B = std::max<int64_t>(1, (int64_t)(budget / (3.0 * (double)npix)));
    if (h->max_batch > 0) B = std::min<int64_t>(B, h->max_batch);
    B = std::min<int64_t>(B, n);
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<3> ev;
    DevArr<uint8_t> d_img(s); DevArr<double> d_R(s), d_t(s); DevArr<int64_t> d_g(s);
    HIPCHK(d_img.alloc(3 * (size_t)npix * (size_t)B));
    HIPCHK(d_R.alloc(9 * (size_t)B)); HIPCHK(d_t.alloc(3 * (size_t)B));
    if (gains) HIPCHK(d_g.alloc(6 * (size_t)B));
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int nb = (int)std::min<int64_t>(B, n - b0);
        ev.rec(0, s);
        HIPCHK(hipMemcpyAsync(d_img, bgr + 3 * npix * b0, 3 * (size_t)npix * nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_R, Rcw + 9 * b0, d_R.bytes(9 * (size_t)nb), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_t, tcw + 3 * b0, d_t.bytes(3 * (size_t)nb), hipMemcpyHostToDevice, s));
        if (gains) HIPCHK(hipMemcpyAsync(d_g, gains + 6 * b0, d_g.bytes(6 * (size_t)nb), hipMemcpyHostToDevice, s));
        ev.rec(1, s);
        if (h->n > 0) {
            const float *depth0 = h->depth ? h->depth->d_depth + ((int64_t)first + b0) * npix : nullptr;
            const auto kernel = gains ? photo_sample_kernel<true> : photo_sample_kernel<false>;
            kernel<<<grid_for(h->n, PHOTO_BLOCK), PHOTO_BLOCK, 0, s>>>(h->n, h->xyz, nb, d_R, d_t, d_img, depth0, h->cam, h->rule, h->width,
                                                                       h->height, h->n_views, h->s1, h->s2,
                                                                       gains ? (const int64_t *)d_g : nullptr);
            HIPCHK(hipGetLastError());
        }
        ev.rec(2, s);
        HIPCHK(hipStreamSynchronize(s));
        h->ms[0] += ev.ms(0, 1); h->ms[1] += ev.ms(1, 2);
        for (int k = 0; k < nb; ++k) h->added[(size_t)first + (size_t)b0 + k] = 1;
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_photo_add_images(lvba_photo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr)
{
    return photo_add_images(h, first, n, Rcw, tcw, bgr, nullptr);
}

extern "C" int32_t lvba_photo_add_images_gains(lvba_photo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw,
                                               const uint8_t *bgr, const int64_t *gains)
{
    return photo_add_images(h, first, n, Rcw, tcw, bgr, gains);
}

extern "C" int32_t lvba_photo_finish(lvba_photo_t h, lvba_photo_summary *summary, int32_t *n_views, uint8_t *rgb, double *sigma)
{
    if (!h || !summary) return lvba_fail(LVBA_ERR_ARG, "null handle or summary");
    lvba_photo_summary out{};
    out.n_points = h->n;
    out.mean_sigma = out.mean_views = NAN;
    out.ms[0] = h->ms[0]; out.ms[1] = h->ms[1]; out.ms[2] = h->ms[2];
    if (h->n == 0) { *summary = out; return LVBA_OK; }
    HIPCHK(hipSetDevice(h->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    const size_t N = (size_t)h->n;
    const unsigned grid = grid_for(h->n, 256);
    EventTimer<2> ev;
    DevArr<uint8_t> d_rgb(s); DevArr<double> d_sigma(s), d_ps(s); DevArr<int32_t> d_pi(s);
    HIPCHK(d_rgb.alloc(3 * N)); HIPCHK(d_sigma.alloc(N)); HIPCHK(d_pi.alloc(3 * (size_t)grid)); HIPCHK(d_ps.alloc((size_t)grid));
    ev.rec(0, s);
    photo_finish_kernel<<<grid, 256, 0, s>>>(h->n, h->n_views, h->s1, h->s2, h->rule.min_views, d_rgb, d_sigma, d_pi, d_ps);
    HIPCHK(hipGetLastError());
    ev.rec(1, s);
    HIPCHK(hipStreamSynchronize(s));
    h->ms[2] += ev.ms(0, 1);
    out.ms[2] = h->ms[2];
    const double t0 = now_ms();
    std::vector<int32_t> pi(3 * (size_t)grid);
    std::vector<double> ps((size_t)grid);
    HIPCHK(d_pi.download(pi.data(), pi.size())); HIPCHK(d_ps.download(ps.data(), ps.size()));
    double sum = 0.0;
    for (size_t k = 0; k < (size_t)grid; ++k) {
        out.n_seen += pi[3 * k]; out.n_valid += pi[3 * k + 1]; out.n_samples += pi[3 * k + 2];
        sum += ps[k];
    }
    if (out.n_valid > 0) out.mean_sigma = sum / (double)out.n_valid;
    if (out.n_seen > 0) out.mean_views = (double)out.n_samples / (double)out.n_seen;
    if (n_views) HIPCHK(h->n_views.download(n_views, N));
    if (rgb) HIPCHK(d_rgb.download(rgb, 3 * N));
    if (sigma) HIPCHK(d_sigma.download(sigma, N));
    out.ms[3] = now_ms() - t0;
    *summary = out;
    return LVBA_OK;
}

extern "C" int32_t lvba_photo_sums(lvba_photo_t h, int32_t *n_views, uint32_t *s1, int64_t *s2)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (h->n == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t N = (size_t)h->n;
    if (n_views) HIPCHK(h->n_views.download(n_views, N));
    if (s1) HIPCHK(h->s1.download(s1, 3 * N));
    if (s2) HIPCHK(h->s2.download(s2, 3 * N));
    return LVBA_OK;
}

extern "C" void lvba_photo_free(lvba_photo_t h)
{
    delete h;
}
