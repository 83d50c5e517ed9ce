// expo.hip -- per-image exposure compensation of the colour fusion: the estimation sums and the solve (lvba_expo_*; the rule is in
// include/lvba_hip.h, its scalar pieces in expo_device.h, also compiled for the host by the tests).  The fusion
// that applies the gains is photo.hip's.
//
// Device design -- the photometric alignment's (palign.hip), with integer sums.  A handle holds the float points, their reference
// colours and validity bytes.  The images of a call come in batches sized by the free memory and stay as the bytes that were
// uploaded.  Per batch two launches:
//   expo_sums_kernel    the hot path.  Grid (chunks, resident images): a workgroup owns one image and EXPO_CHUNK consecutive points
//                       -- a compile-time constant.  Pose, gains, image base and depth base depend on blockIdx.y alone:
//                       workgroup-uniform, scalar loads.  Lane l takes the points chunk * EXPO_CHUNK + l + k * 256 in index order
//                       and keeps the 20 counters in registers: 32 bits for the counts and the first-order sums of its 16 points,
//                       64 for the products.  Then the DPP tree of wave_ops.h -- in 32 bits where a workgroup's total fits them
//                       (4096 65280 < 2^29), in 64 for the products --, the four wavefronts' shares added through LDS, one
//                       partial [image][chunk][20].
//   expo_reduce_kernel  one wavefront per image: lane q adds the image's partials of sum q in chunk order.
// The sums are integers: the order of the additions is of no account, and nothing depends on the batching.  No atomics: the
// second form the sums could take -- one 64-bit atomic per sum and workgroup -- was not built.
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
#include "wave_ops.h"
#include "expo_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

static_assert(LVBA_EXPO_OK == EXPO_OK && LVBA_EXPO_FALLBACK_GAIN == EXPO_FALLBACK_GAIN && LVBA_EXPO_TOO_FEW_SAMPLES == EXPO_TOO_FEW &&
              LVBA_EXPO_OUT_OF_BOUNDS == EXPO_OUT_OF_BOUNDS, "exposure states");
static_assert(LVBA_EXPO_AFFINE == EXPO_AFFINE && LVBA_EXPO_GAIN == EXPO_GAIN, "exposure models");
static_assert(LVBA_EXPO_SUMS == EXPO_NS, "the sums of lvba_expo_sums");
static_assert(EXPO_BLOCK == 256 && EXPO_CHUNK % EXPO_BLOCK == 0, "the sums kernel adds four wavefronts' shares over whole rounds");
static_assert((int64_t)EXPO_CHUNK * EXPO_C_MAX < ((int64_t)1 << 31), "a workgroup's first-order sums are reduced in 32 bits");

struct lvba_expo_s {
    int device = 0;
    int64_t n = 0;
    int n_images = 0, width = 0, height = 0;
    TrkIntr cam{};
    PhotoRule rule{};
    ExpoRule expo{};
    int32_t max_batch = 0;
    lvba_depth_t depth = nullptr;  // the caller's, kept alive by the caller
    // handle-owned device arrays (no stream: every call has drained its own before it returned)
    DevArr<float> xyz;             // [n][3]
    DevArr<uint16_t> ref16;        // [n][3]
    DevArr<uint8_t> valid;         // [n]
    double ms[2] = {0, 0};         // upload, sums pass: accumulated
    ~lvba_expo_s()
    {
        (void)hipSetDevice(device);
        xyz.reset(); ref16.reset(); valid.reset();
    }
};

namespace {

// images 0 .. gridDim.y - 1 of the batch: Rcw [B][9], tcw [B][3], gains [B][3][2] (null: identity), bgr [B][H][W][3] as uploaded;
// depth0 = the depth image of the batch's first image (null: no occlusion test).  part [B][gridDim.x][EXPO_NS];
// gridDim.x = expo_chunks(n).
__global__ __launch_bounds__(EXPO_BLOCK, 2) void expo_sums_kernel(int64_t n, const float *__restrict__ xyz, const uint16_t *__restrict__ ref16,
                                                                  const uint8_t *__restrict__ valid, const double *__restrict__ Rcw,
                                                                  const double *__restrict__ tcw, const int64_t *__restrict__ gains,
                                                                  const uint8_t *__restrict__ bgr, const float *__restrict__ depth0,
                                                                  const TrkIntr cam, const PhotoRule o, const ExpoRule e, int W, int H,
                                                                  uint64_t *__restrict__ part)
{
    __shared__ uint64_t red[EXPO_BLOCK / 64][EXPO_NS];
    const int img = blockIdx.y;
    double R[9], t[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = Rcw[9 * (int64_t)img + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = tcw[3 * (int64_t)img + q];
    int64_t g[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) g[q] = gains ? gains[6 * (int64_t)img + q] : ((q & 1) ? 0 : EXPO_ONE);
    const int64_t npix = (int64_t)W * H;
    const uint8_t *__restrict__ tb = bgr + 3 * (int64_t)img * npix;
    const float *__restrict__ db = depth0 ? depth0 + (int64_t)img * npix : nullptr;
    ExpoAcc acc;
    expo_acc_zero(acc);
    const int64_t base = (int64_t)blockIdx.x * EXPO_CHUNK + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < EXPO_CHUNK / EXPO_BLOCK; ++k) {
        const int64_t i = base + (int64_t)k * EXPO_BLOCK;
        if (i >= n) break;
        if (!valid[i]) continue;
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        expo_point(cam, db, W, H, R, t, X, ref16 + 3 * i, o, e, g,
                   [&](int y, int x) { return photo_texel_of(tb + 3 * ((int64_t)y * W + x)); }, acc);
    }
    // the 20 sums in the order of the result: the counts and first-order sums through the 32-bit tree, the products through the 64-bit one
    uint64_t s[EXPO_NS];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[EXPO_PER * k + 0] = (uint32_t)wave_fold_to_lane63<SumStepI32>((int)acc.n[k]);
        s[EXPO_PER * k + 1] = (uint32_t)wave_fold_to_lane63<SumStepI32>((int)acc.sc[k]);
        s[EXPO_PER * k + 2] = (uint32_t)wave_fold_to_lane63<SumStepI32>((int)acc.sr[k]);
        s[EXPO_PER * k + 3] = wave_fold_to_lane63<SumStepI64>((unsigned long long)acc.scc[k]);
        s[EXPO_PER * k + 4] = wave_fold_to_lane63<SumStepI64>((unsigned long long)acc.scr[k]);
        s[EXPO_PER * k + 5] = wave_fold_to_lane63<SumStepI64>((unsigned long long)acc.see[k]);
    }
    s[EXPO_LOCATED] = (uint32_t)wave_fold_to_lane63<SumStepI32>((int)acc.located);
    s[EXPO_REFUSED] = (uint32_t)wave_fold_to_lane63<SumStepI32>((int)acc.refused);
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < EXPO_NS; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < EXPO_NS) {
        const int q = threadIdx.x;
        part[((int64_t)img * gridDim.x + blockIdx.x) * EXPO_NS + q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
    }
}

// nc: the sums kernel's gridDim.x.  sums [B][EXPO_NS]
__global__ __launch_bounds__(64) void expo_reduce_kernel(int64_t nc, const uint64_t *__restrict__ part, uint64_t *__restrict__ sums)
{
    const int img = blockIdx.x;
    if (threadIdx.x >= EXPO_NS) return;
    const uint64_t *__restrict__ P = part + (int64_t)img * nc * EXPO_NS + threadIdx.x;
    uint64_t a = 0;
    for (int64_t b = 0; b < nc; ++b) a += P[b * EXPO_NS];
    sums[(int64_t)img * EXPO_NS + threadIdx.x] = a;
}

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// the options with the defaults under them, checked; the solve's integers out
int32_t check_opts(const lvba_expo_opts *opts, lvba_expo_opts &o, ExpoSolveRule &r)
{
    lvba_expo_default_opts(&o);
    if (opts) o = *opts;
    if (!finite_nonneg(o.occlusion_rel) || !finite_nonneg(o.occlusion_abs) || !finite_nonneg(o.max_depth) || o.max_batch_images < 0)
        return lvba_fail(LVBA_ERR_ARG, "options: occlusion_rel %g, occlusion_abs %g, max_depth %g (finite, >= 0), max_batch_images %d (>= 0)",
                         o.occlusion_rel, o.occlusion_abs, o.max_depth, o.max_batch_images);
    if (o.model != LVBA_EXPO_AFFINE && o.model != LVBA_EXPO_GAIN) return lvba_fail(LVBA_ERR_ARG, "model %d (LVBA_EXPO_AFFINE or LVBA_EXPO_GAIN)", o.model);
    if (o.sat_lo < 0 || o.sat_hi > 255 || o.sat_lo > o.sat_hi) return lvba_fail(LVBA_ERR_ARG, "sat_lo %d, sat_hi %d (0 <= sat_lo <= sat_hi <= 255)", o.sat_lo, o.sat_hi);
    if (o.gate < 0 || o.gate > 255) return lvba_fail(LVBA_ERR_ARG, "gate %d grey levels (0 .. 255)", o.gate);
    if (o.min_samples < 2) return lvba_fail(LVBA_ERR_ARG, "min_samples %d (>= 2)", o.min_samples);
    if (o.min_spread < 0 || o.min_spread > 255) return lvba_fail(LVBA_ERR_ARG, "min_spread %d grey levels (0 .. 255)", o.min_spread);
    if (!(o.min_gain >= 0.25 && o.min_gain <= 1.0 && o.max_gain >= 1.0 && o.max_gain <= 4.0) || !(o.max_offset >= 0.0 && o.max_offset <= 255.0))
        return lvba_fail(LVBA_ERR_ARG, "options: min_gain %g (0.25 .. 1), max_gain %g (1 .. 4), max_offset %g grey levels (0 .. 255)", o.min_gain,
                         o.max_gain, o.max_offset);
    r = ExpoSolveRule{o.model, o.min_samples, o.min_spread, 0, (int64_t)std::floor(o.min_gain * 65536.0 + 0.5),
                      (int64_t)std::floor(o.max_gain * 65536.0 + 0.5), (int64_t)std::floor(o.max_offset * 16777216.0 + 0.5)};
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_expo_default_opts(lvba_expo_opts *o)
{
    if (!o) return;
    *o = lvba_expo_opts{};
    o->occlusion_rel = 0.05; o->occlusion_abs = 0.1; o->max_depth = 0.0; // the colour fusion's
    // this library's choice, none tuned on recorded data
    o->min_gain = 0.25; o->max_gain = 4.0; o->max_offset = 64.0;
    o->holes = 0; o->model = LVBA_EXPO_AFFINE; o->sat_lo = 4; o->sat_hi = 251; o->gate = 30; o->min_samples = 200; o->min_spread = 2;
    o->max_batch_images = 0;
}

extern "C" int32_t lvba_expo_create(int32_t device, int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int32_t n_images,
                                    int32_t width, int32_t height, const double *intr, lvba_depth_t depth, const lvba_expo_opts *opts,
                                    lvba_expo_t *out)
{
    if (!out) return lvba_fail(LVBA_ERR_ARG, "null output");
    if (!intr || (n > 0 && (!xyz || !ref16 || !valid))) return lvba_fail(LVBA_ERR_ARG, "null points, references, validity or intrinsics");
    if (n < 0 || n >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_ARG, "%lld points (0 .. 2^32 - 1)", (long long)n);
    if (width < 2 || height < 2) return lvba_fail(LVBA_ERR_ARG, "image size %d x %d (both must be >= 2)", width, height);
    if (n_images < 1 || n_images > PHOTO_MAX_IMAGES) return lvba_fail(LVBA_ERR_ARG, "%d images (1 .. %d)", n_images, PHOTO_MAX_IMAGES);
    if (depth && (depth->n_images != n_images || depth->width != width || depth->height != height || depth->device != device))
        return lvba_fail(LVBA_ERR_ARG, "depth set of %d images of %d x %d on device %d; the images are %d of %d x %d on device %d",
                         depth->n_images, depth->width, depth->height, depth->device, n_images, width, height, device);
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    lvba_expo_opts o;
    ExpoSolveRule unused;
    TRY(check_opts(opts, o, unused));
    if (n > 0)
        for (int64_t i = 0; i < 3 * n; ++i)
            if (ref16[i] > EXPO_C_MAX) return lvba_fail(LVBA_ERR_ARG, "reference %u of point %lld (at most 65 280)", (unsigned)ref16[i], (long long)(i / 3));
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_expo_s *h = new (std::nothrow) lvba_expo_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    struct Guard { lvba_expo_s *h; ~Guard() { delete h; } } guard{h};
    h->device = device; h->n = n; h->n_images = n_images; h->width = width; h->height = height;
    h->cam = trk_intr_of(intr);
    h->rule = photo_rule_of(depth != nullptr, o.occlusion_rel, o.occlusion_abs, o.max_depth, o.holes, 2);
    h->expo = ExpoRule{o.sat_lo, o.sat_hi, o.gate * 256, 0};
    h->max_batch = o.max_batch_images;
    h->depth = depth;
    const size_t N = (size_t)n;
    HIPCHK(h->xyz.alloc(3 * N)); HIPCHK(h->ref16.alloc(3 * N)); HIPCHK(h->valid.alloc(N));
    if (n > 0) {
        HIPCHK(h->xyz.upload(xyz, 3 * N)); HIPCHK(h->ref16.upload(ref16, 3 * N)); HIPCHK(h->valid.upload(valid, N));
        HIPCHK(hipDeviceSynchronize());
    }
    *out = h;
    guard.h = nullptr;
    return LVBA_OK;
}

extern "C" int32_t lvba_expo_sums(lvba_expo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                                  const int64_t *gains_in, uint64_t *sums)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (first < 0 || n < 0 || (int64_t)first + n > h->n_images || (n > 0 && first >= h->n_images))
        return lvba_fail(LVBA_ERR_ARG, "images [%d, %d + %d) of %d", first, first, n, h->n_images);
    if (n > 0 && (!Rcw || !tcw || !bgr || !sums)) return lvba_fail(LVBA_ERR_ARG, "null cameras, images or output");
    if (n == 0) return LVBA_OK;
    TRY(check_rotations_finite(Rcw, 0, n));
    TRY(check_translations_finite(tcw, 0, n));
    if (gains_in && !expo_gains_ok(gains_in, 3 * (int64_t)n))
        return lvba_fail(LVBA_ERR_ARG, "gains: A outside [2^14, 2^18] or |B| above 2^16 * 65280");
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)h->width * h->height;
    const int64_t nc = expo_chunks(h->n);
    // the batch: the uploaded bytes, the partials and the sums of B images
    const double per_image = 3.0 * (double)npix + ((double)nc + 1.0) * EXPO_NS * sizeof(uint64_t) + 18.0 * sizeof(double);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(0.4 * ((double)free_b + (double)DevicePool::get().cached_bytes()), 8.0 * (1 << 30));
    int64_t B = std::max<int64_t>(1, (int64_t)(budget / per_image));
    if (h->max_batch > 0) B = std::min<int64_t>(B, h->max_batch);
    B = std::min<int64_t>(B, n); // (<= 32 768: within gridDim.y)
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<3> ev;
    DevArr<uint8_t> d_img(s); DevArr<double> d_R(s), d_t(s); DevArr<int64_t> d_g(s); DevArr<uint64_t> d_part(s), d_sums(s);
    HIPCHK(d_img.alloc(3 * (size_t)npix * (size_t)B));
    HIPCHK(d_R.alloc(9 * (size_t)B)); HIPCHK(d_t.alloc(3 * (size_t)B)); HIPCHK(d_g.alloc(6 * (size_t)B));
    HIPCHK(d_part.alloc((size_t)EXPO_NS * (size_t)nc * (size_t)B)); HIPCHK(d_sums.alloc((size_t)EXPO_NS * (size_t)B));
    std::vector<uint64_t> hsums((size_t)EXPO_NS * (size_t)n, 0); // the caller's array is written once, at the end
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int nb = (int)std::min<int64_t>(B, n - b0);
        if (h->n == 0) break; // no point: every sum is 0
        ev.rec(0, s);
        HIPCHK(hipMemcpyAsync(d_img, bgr + 3 * npix * b0, 3 * (size_t)npix * nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_R, Rcw + 9 * b0, d_R.bytes(9 * (size_t)nb), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_t, tcw + 3 * b0, d_t.bytes(3 * (size_t)nb), hipMemcpyHostToDevice, s));
        if (gains_in) HIPCHK(hipMemcpyAsync(d_g, gains_in + 6 * b0, d_g.bytes(6 * (size_t)nb), hipMemcpyHostToDevice, s));
        ev.rec(1, s);
        const float *depth0 = h->depth ? h->depth->d_depth + ((int64_t)first + b0) * npix : nullptr;
        expo_sums_kernel<<<dim3((unsigned)nc, (unsigned)nb), EXPO_BLOCK, 0, s>>>(h->n, h->xyz, h->ref16, h->valid, d_R, d_t,
                                                                                 gains_in ? (const int64_t *)d_g : nullptr, d_img, depth0, h->cam,
                                                                                 h->rule, h->expo, h->width, h->height, d_part);
        HIPCHK(hipGetLastError());
        expo_reduce_kernel<<<(unsigned)nb, 64, 0, s>>>(nc, d_part, d_sums);
        HIPCHK(hipGetLastError());
        ev.rec(2, s);
        HIPCHK(hipStreamSynchronize(s));
        h->ms[0] += ev.ms(0, 1); h->ms[1] += ev.ms(1, 2);
        HIPCHK(d_sums.download(hsums.data() + (size_t)EXPO_NS * (size_t)b0, (size_t)EXPO_NS * (size_t)nb));
    }
    std::copy(hsums.begin(), hsums.end(), sums);
    return LVBA_OK;
}

extern "C" int32_t lvba_expo_solve(int32_t n_images, const uint64_t *sums, const lvba_expo_opts *opts, int64_t *gains, int32_t *status)
{
    if (n_images < 0 || n_images > PHOTO_MAX_IMAGES) return lvba_fail(LVBA_ERR_ARG, "%d images (0 .. %d)", n_images, PHOTO_MAX_IMAGES);
    if (n_images > 0 && (!sums || !gains || !status)) return lvba_fail(LVBA_ERR_ARG, "null sums or output");
    lvba_expo_opts o;
    ExpoSolveRule r;
    TRY(check_opts(opts, o, r));
    // sums an image of fewer than 2^32 points can have: the solve's 128-bit products rest on them
    for (int64_t q = 0; q < (int64_t)n_images * 3; ++q) {
        const uint64_t *c = sums + EXPO_NS * (q / 3) + EXPO_PER * (q % 3);
        const uint64_t lim = c[0] * (uint64_t)EXPO_C_MAX;
        if (c[0] >= ((uint64_t)1 << 32) || c[1] > lim || c[2] > lim || c[3] > lim * EXPO_C_MAX || c[4] > lim * EXPO_C_MAX)
            return lvba_fail(LVBA_ERR_ARG, "sums of image %lld, channel %d: not those of fewer than 2^32 samples of at most 65 280", (long long)(q / 3),
                             (int)(q % 3));
    }
    if (n_images > 0) expo_solve(n_images, sums, r, gains, status);
    return LVBA_OK;
}

extern "C" int32_t lvba_expo_profile(lvba_expo_t h, double *ms)
{
    if (!h || !ms) return lvba_fail(LVBA_ERR_ARG, "null handle or output");
    ms[0] = h->ms[0]; ms[1] = h->ms[1];
    return LVBA_OK;
}

extern "C" void lvba_expo_free(lvba_expo_t h)
{
    delete h;
}
