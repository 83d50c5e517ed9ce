// palign.hip -- photometric camera alignment against the coloured map (lvba_palign_*; the rule is in include/lvba_hip.h, its
// scalar pieces in palign_device.h, also compiled for the host by the tests).
//
// Device design -- the extrinsic refinement's (calib.hip), the reduction being per image, not per point.  A handle holds the float
// points, their reference colours and validity bytes.  The images of a call come in batches sized by the free memory, stay as the
// bytes that were uploaded and stay resident for all their iterations: the images are independent given a fixed reference, so a
// batch runs its complete iteration before the next one is uploaded.  Per pass two launches and one word read by the host:
//   palign_linearize_kernel  the hot path.  Grid (chunks, resident images): a workgroup owns one image and PAL_CHUNK consecutive
//                            points -- a compile-time constant, so an image's bytes depend neither on the device nor on what else
//                            is resident.  Pose, image base and depth base depend on blockIdx.y alone: workgroup-uniform, scalar
//                            loads.  Lane l takes the points chunk * PAL_CHUNK + l + k * 256 in index order (coalesced loads of
//                            12 + 6 + 1 bytes a point) and keeps the PAL_NS sums in vector registers; the integer texel
//                            arithmetic is photo_sample_kernel's, the fp64 work the projection, its Jacobian and the row
//                            products.  Then the fixed tree of wave_ops.h, the four wavefronts' shares added in index order
//                            through LDS, one partial [image][chunk][PAL_NS].  No atomics: the bytes do not change run to run.
//                            The workgroups of a finished image return at once on the image's status.
//   palign_step_kernel       one wavefront per image: lane q adds the image's partials of sum q in chunk order; lane 0 takes the
//                            accept / reject decision, solves the damped system (6 x 6 LDL^T in registers), writes the next
//                            trial pose and the status.  An image that goes on sets the pass's word in the host's pinned memory.
// There is no per-image candidate list: DESIGN.md §10q prices it.
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
#include "palign_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

static_assert(LVBA_PALIGN_CONVERGED == PAL_CONVERGED && LVBA_PALIGN_MAX_ITERATIONS == PAL_MAX_ITERATIONS &&
              LVBA_PALIGN_TOO_FEW_SAMPLES == PAL_TOO_FEW && LVBA_PALIGN_DEGENERATE == PAL_DEGENERATE &&
              LVBA_PALIGN_OUT_OF_BOUNDS == PAL_OUT_OF_BOUNDS, "alignment states");
static_assert(PAL_BLOCK == 256 && PAL_CHUNK % PAL_BLOCK == 0, "the linearisation adds four wavefronts' shares over whole rounds");
static_assert(LVBA_PALIGN_SUMS == PAL_NS, "the sums of lvba_palign_linearize");

struct lvba_palign_s {
    int device = 0;
    int64_t n = 0;
    int n_images = 0, width = 0, height = 0;
    TrkIntr cam{};
    PhotoRule rule{};
    PalParams par{};
    int32_t max_batch = 0;
    lvba_depth_t depth = nullptr;  // the caller's, kept alive by the caller
    // handle-owned device arrays (no stream: every call has drained its own before it returned)
    DevArr<float> xyz;             // [n][3]
    DevArr<uint16_t> ref16;        // [n][3]
    DevArr<uint8_t> valid;         // [n]
    double ms[3] = {0, 0, 0};      // upload, linearisation passes, steps: accumulated
    ~lvba_palign_s()
    {
        (void)hipSetDevice(device);
        xyz.reset(); ref16.reset(); valid.reset();
    }
};

namespace {

// images 0 .. gridDim.y - 1 of the batch: state [B], bgr [B][H][W][3] as uploaded; depth0 = the depth image of the batch's first
// image (null: no occlusion test).  part [B][gridDim.x][PAL_NS]; gridDim.x = pal_chunks(n).
__global__ __launch_bounds__(PAL_BLOCK, 2) void palign_linearize_kernel(int64_t n, const float *__restrict__ xyz, const uint16_t *__restrict__ ref16,
                                                                     const uint8_t *__restrict__ valid, const PalState *__restrict__ state,
                                                                     const uint8_t *__restrict__ bgr, const float *__restrict__ depth0,
                                                                     const TrkIntr cam, const PhotoRule o, int loss_kind, double loss_scale,
                                                                     int W, int H, double *__restrict__ part)
{
    __shared__ double red[PAL_BLOCK / 64][PAL_NS];
    const int img = blockIdx.y;
    const PalState &st = state[img];
    if (st.status != PAL_RUNNING) return;
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = st.Rt[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = st.tt[e];
    const int64_t npix = (int64_t)W * H;
    const uint8_t *__restrict__ tb = bgr + 3 * (int64_t)img * npix;
    const float *__restrict__ db = depth0 ? depth0 + (int64_t)img * npix : nullptr;
    double s[PAL_NS];
#pragma unroll
    for (int q = 0; q < PAL_NS; ++q) s[q] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * PAL_CHUNK + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < PAL_CHUNK / PAL_BLOCK; ++k) {
        const int64_t i = base + (int64_t)k * PAL_BLOCK;
        if (i >= n) break;
        if (!valid[i]) continue;
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        pal_point(cam, db, W, H, R, t, X, ref16 + 3 * i, o, loss_kind, loss_scale,
                  [&](int y, int x) { return photo_texel_of(tb + 3 * ((int64_t)y * W + x)); }, s);
    }
#pragma unroll
    for (int q = 0; q < PAL_NS; ++q) s[q] = wave_sum_to_lane63(s[q]); // (a lane without a source adds 0.0)
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < PAL_NS; ++q) red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < PAL_NS) {
        const int q = threadIdx.x;
        part[((int64_t)img * gridDim.x + blockIdx.x) * PAL_NS + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// nc: the linearisation's gridDim.x.  sums_only: lvba_palign_linearize (no step): sums [B][PAL_NS] out.  flag: the host's word of
// this pass, set by every image that goes on.
__global__ __launch_bounds__(64) void palign_step_kernel(int64_t nc, const double *__restrict__ part, const PalParams o, int sums_only,
                                                         PalState *__restrict__ state, double *__restrict__ sums, int32_t *__restrict__ flag)
{
    __shared__ double sh[PAL_NS];
    const int img = blockIdx.x;
    if (state[img].status != PAL_RUNNING) return;
    if (threadIdx.x < PAL_NS) {
        // the partials added one after another in chunk order: the loads go out sixteen at a time, the order of the additions stays
        const double *__restrict__ P = part + (int64_t)img * nc * PAL_NS + threadIdx.x;
        double a = 0.0;
        int64_t b = 0;
        for (; b + 16 <= nc; b += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = P[(b + k) * PAL_NS];
#pragma unroll
            for (int k = 0; k < 16; ++k) a += v[k];
        }
        for (; b < nc; ++b) a += P[b * PAL_NS];
        sh[threadIdx.x] = a;
        if (sums_only) sums[(int64_t)img * PAL_NS + threadIdx.x] = a;
    }
    __syncthreads();
    if (sums_only || threadIdx.x != 0) return;
    double s[PAL_NS];
    for (int q = 0; q < PAL_NS; ++q) s[q] = sh[q];
    const int st = pal_step(s, o, state[img]);
    if (st == PAL_RUNNING) *flag = 1;
    else state[img].status = st;
}

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

int32_t check_opts(const lvba_palign_opts *opts, lvba_palign_opts &o)
{
    lvba_palign_default_opts(&o);
    if (opts) o = *opts;
    if (!finite_nonneg(o.occlusion_rel) || !finite_nonneg(o.occlusion_abs) || !finite_nonneg(o.max_depth) || o.max_batch_images < 0)
        return lvba_fail(LVBA_ERR_ARG, "options: occlusion_rel %g, occlusion_abs %g, max_depth %g (finite, >= 0), max_batch_images %d (>= 0)",
                         o.occlusion_rel, o.occlusion_abs, o.max_depth, o.max_batch_images);
    if (o.max_iterations < 1 || o.max_iterations > 1000) return lvba_fail(LVBA_ERR_ARG, "max_iterations %d (1 .. 1000)", o.max_iterations);
    if (o.min_samples < 6) return lvba_fail(LVBA_ERR_ARG, "min_samples %d (>= 6)", o.min_samples);
    if (!finite_nonneg(o.eps_rot) || !finite_nonneg(o.eps_trans) || !finite_nonneg(o.max_rotation_deg) || !finite_nonneg(o.max_translation) ||
        o.max_rotation_deg > 180.0)
        return lvba_fail(LVBA_ERR_ARG, "options: eps_rot %g, eps_trans %g, max_rotation_deg %g (<= 180), max_translation %g (finite, >= 0)",
                         o.eps_rot, o.eps_trans, o.max_rotation_deg, o.max_translation);
    if (o.loss_kind < LVBA_LOSS_TRIVIAL || o.loss_kind > LVBA_LOSS_TUKEY || !(o.loss_scale > 0.0 && std::isfinite(o.loss_scale)))
        return lvba_fail(LVBA_ERR_ARG, "loss: kind %d, scale %g grey levels (a known kind; finite and > 0)", o.loss_kind, o.loss_scale);
    return LVBA_OK;
}

// Both entry points.  sums_out: one linearisation per image at the given poses, sums [n][PAL_NS] out; else the iteration and every
// per-image output of lvba_palign_align.  Nothing is written before the arguments have passed.
int32_t palign_run(lvba_palign_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr, double *sums_out,
                   double *Rcw_out, double *tcw_out, int32_t *status, int32_t *iterations, int32_t *accepted, int64_t *n_samples,
                   double *rmse_initial, double *rmse, double *cost, double *information)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (first < 0 || n < 0 || (int64_t)first + n > h->n_images || (n > 0 && first >= h->n_images))
        return lvba_fail(LVBA_ERR_ARG, "images [%d, %d + %d) of %d", first, first, n, h->n_images);
    const bool sums_only = sums_out != nullptr;
    if (n > 0 && (!Rcw || !tcw || !bgr)) return lvba_fail(LVBA_ERR_ARG, "null cameras or images");
    if (!sums_only && n > 0 && !(Rcw_out && tcw_out && status && iterations && accepted && n_samples && rmse_initial && rmse && cost && information))
        return lvba_fail(LVBA_ERR_ARG, "null output");
    if (n == 0) return LVBA_OK;
    TRY(check_rotations_finite(Rcw, 0, n));
    TRY(check_translations_finite(tcw, 0, n));
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)h->width * h->height;
    const int64_t nc = pal_chunks(h->n);
    // the batch: the uploaded bytes, the partials and the state of B images
    const double per_image = 3.0 * (double)npix + (double)nc * PAL_NS * sizeof(double) + (double)sizeof(PalState) + PAL_NS * sizeof(double);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(0.4 * ((double)free_b + (double)DevicePool::get().cached_bytes()), 8.0 * (1 << 30));
    int64_t B = std::max<int64_t>(1, (int64_t)(budget / per_image));
    if (h->max_batch > 0) B = std::min<int64_t>(B, h->max_batch);
    B = std::min<int64_t>(B, n);
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    PinnedWords words;
    HIPCHK(PinnedCache::get().acquire((void **)&words.p, 4096)); // (>= 1000 words; one size for the cache's sake)
    int32_t *d_words = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&d_words, words.p, 0));
    EventTimer<4> ev;
    DevArr<uint8_t> d_img(s); DevArr<PalState> d_state(s); DevArr<double> d_part(s), d_sums(s);
    HIPCHK(d_img.alloc(3 * (size_t)npix * (size_t)B));
    HIPCHK(d_state.alloc((size_t)B)); HIPCHK(d_part.alloc((size_t)PAL_NS * (size_t)nc * (size_t)B)); HIPCHK(d_sums.alloc((size_t)PAL_NS * (size_t)B));
    std::vector<PalState> hstate((size_t)B);
    std::vector<double> hsums(sums_only ? (size_t)PAL_NS * (size_t)B : 0);
    const int passes = sums_only ? 1 : h->par.max_iterations;
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int nb = (int)std::min<int64_t>(B, n - b0);
        for (int k = 0; k < nb; ++k) pal_state_init(hstate[(size_t)k], Rcw + 9 * (b0 + k), tcw + 3 * (b0 + k));
        for (int it = 0; it < passes; ++it) words.p[it] = 0;
        ev.rec(0, s);
        HIPCHK(hipMemcpyAsync(d_img, bgr + 3 * npix * b0, 3 * (size_t)npix * nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_state, hstate.data(), d_state.bytes((size_t)nb), hipMemcpyHostToDevice, s));
        ev.rec(1, s);
        HIPCHK(hipStreamSynchronize(s));
        h->ms[0] += ev.ms(0, 1);
        const float *depth0 = h->depth ? h->depth->d_depth + ((int64_t)first + b0) * npix : nullptr;
        for (int it = 0; it < passes; ++it) {
            ev.rec(1, s);
            palign_linearize_kernel<<<dim3((unsigned)nc, (unsigned)nb), PAL_BLOCK, 0, s>>>(h->n, h->xyz, h->ref16, h->valid, d_state, d_img, depth0,
                                                                                        h->cam, h->rule, h->par.loss_kind, h->par.loss_scale,
                                                                                        h->width, h->height, d_part);
            HIPCHK(hipGetLastError());
            ev.rec(2, s);
            palign_step_kernel<<<(unsigned)nb, 64, 0, s>>>(nc, d_part, h->par, sums_only ? 1 : 0, d_state, d_sums, d_words + it);
            HIPCHK(hipGetLastError());
            ev.rec(3, s);
            HIPCHK(hipStreamSynchronize(s));
            h->ms[1] += ev.ms(1, 2); h->ms[2] += ev.ms(2, 3);
            if (!words.p[it]) break; // every image of the batch has finished
        }
        if (sums_only) {
            HIPCHK(d_sums.download(hsums.data(), (size_t)PAL_NS * (size_t)nb));
            std::copy_n(hsums.data(), (size_t)PAL_NS * (size_t)nb, sums_out + (size_t)PAL_NS * (size_t)b0);
            continue;
        }
        HIPCHK(d_state.download(hstate.data(), (size_t)nb));
        for (int k = 0; k < nb; ++k) {
            const PalState &st = hstate[(size_t)k];
            const size_t j = (size_t)(b0 + k);
            std::copy_n(st.R, 9, Rcw_out + 9 * j);
            std::copy_n(st.t, 3, tcw_out + 3 * j);
            status[j] = st.status; iterations[j] = st.passes; accepted[j] = st.accepted;
            n_samples[j] = (int64_t)st.cur[PAL_CNT];
            rmse_initial[j] = st.first[PAL_CNT] > 0.0 ? sqrt(st.first[PAL_SSQ] / (3.0 * st.first[PAL_CNT])) : 0.0;
            rmse[j] = st.cur[PAL_CNT] > 0.0 ? sqrt(st.cur[PAL_SSQ] / (3.0 * st.cur[PAL_CNT])) : 0.0;
            cost[j] = st.cur[PAL_COST];
            pal_expand(st.cur, information + 36 * j);
        }
    }
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_palign_default_opts(lvba_palign_opts *o)
{
    if (!o) return;
    *o = lvba_palign_opts{};
    o->occlusion_rel = 0.05; o->occlusion_abs = 0.1; o->max_depth = 0.0; // the colour fusion's
    o->loss_scale = 10.0;          // the prototype's value, not tuned on recorded data
    o->eps_rot = 1e-7; o->eps_trans = 1e-6;
    o->max_rotation_deg = 5.0; o->max_translation = 0.5;
    o->holes = 0; o->loss_kind = LVBA_LOSS_HUBER; o->min_samples = 200; o->max_iterations = 15; o->max_batch_images = 0; o->reserved = 0;
}

extern "C" int32_t lvba_palign_create(int32_t device, int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid,
                                      int32_t n_images, int32_t width, int32_t height, const double *intr, lvba_depth_t depth,
                                      const lvba_palign_opts *opts, lvba_palign_t *out)
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
    lvba_palign_opts o;
    TRY(check_opts(opts, o));
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_palign_s *h = new (std::nothrow) lvba_palign_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    struct Guard { lvba_palign_s *h; ~Guard() { delete h; } } guard{h};
    h->device = device; h->n = n; h->n_images = n_images; h->width = width; h->height = height;
    h->cam = trk_intr_of(intr);
    h->rule = photo_rule_of(depth != nullptr, o.occlusion_rel, o.occlusion_abs, o.max_depth, o.holes, 2);
    const double half = 0.5 * o.max_rotation_deg * (M_PI / 180.0);
    h->par = PalParams{o.loss_scale, o.eps_rot, o.eps_trans, 8.0 * std::sin(half) * std::sin(half), o.max_translation, o.loss_kind, o.min_samples,
                       o.max_iterations, 0};
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

extern "C" int32_t lvba_palign_linearize(lvba_palign_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                                         double *sums)
{
    if (!sums && n > 0) return lvba_fail(LVBA_ERR_ARG, "null output");
    double none = 0.0;
    return palign_run(h, first, n, Rcw, tcw, bgr, sums ? sums : &none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr);
}

extern "C" int32_t lvba_palign_align(lvba_palign_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                                     double *Rcw_out, double *tcw_out, int32_t *status, int32_t *iterations, int32_t *accepted,
                                     int64_t *n_samples, double *rmse_initial, double *rmse, double *cost, double *information)
{
    return palign_run(h, first, n, Rcw, tcw, bgr, nullptr, Rcw_out, tcw_out, status, iterations, accepted, n_samples, rmse_initial, rmse, cost,
                      information);
}

extern "C" int32_t lvba_palign_profile(lvba_palign_t h, double *ms)
{
    if (!h || !ms) return lvba_fail(LVBA_ERR_ARG, "null handle or output");
    ms[0] = h->ms[0]; ms[1] = h->ms[1]; ms[2] = h->ms[2];
    return LVBA_OK;
}

extern "C" void lvba_palign_free(lvba_palign_t h)
{
    delete h;
}
