// undistort.hip -- the undistorted images of the COLMAP export (lvba_undistort_*; the rule is in include/lvba_hip.h, its scalar
// pieces in undistort_device.h, also compiled for the host by the tests).
//
// Device design.  A handle holds the source camera, the target pinhole and the two sizes; it owns no device memory.  The images
// of a call go up, and the undistorted ones come back, in batches of at most max_batch_images (0: sized by the free memory, as
// photo.hip sizes its own); per batch one launch of
//   undistort_kernel     the hot path.  The grid runs over (tile of the target, image of the batch); a workgroup of 256 lanes owns
//                        a tile of 64 x 16 target pixels, a lane four consecutive pixels of a row.  The camera, the pinhole and
//                        the sizes are kernel arguments and the image's six gains are read through a workgroup-uniform address:
//                        all of them sit in scalar registers.  A lane recomputes the source position of each of its pixels
//                        (about 40 fp64 operations; no map is kept in memory), reads the four texels about it as bytes from the
//                        uploaded image -- the map is smooth, so neighbouring lanes share cache lines --, and packs its twelve
//                        output bytes into three dwords.  An image's base k * w' * h' * 3 and a row's start need not be a
//                        multiple of four: the lane stores the dwords that lie aligned inside its twelve bytes (three, or two)
//                        and the bytes before and after them one by one; a lane cut by the image's right edge stores bytes.
//                        No atomics, no LDS, no synchronisation.
//   undistort_map_kernel one lane per target pixel over the same und_locate: (u, v) or NaN, and the mask byte.  It runs once at
//                        create (the mask alone, for n_valid) and in lvba_undistort_map.
// Every pixel is a function of its own image, the cameras and the image's gains: nothing depends on the batching.
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
#include "undistort_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

struct lvba_undistort_s {
    int device = 0;
    int width = 0, height = 0, out_width = 0, out_height = 0;
    TrkIntr cam{};
    UndPinhole pin{};
    uint32_t border = 0;
    int32_t max_batch = 0;
    int64_t n_valid = 0;
    double ms[3] = {0, 0, 0}; // upload, kernel, download: accumulated
};

namespace {

// src [B][H][W][3] as uploaded, dst [B][Ho][Wo][3]; gains [B][3][2] (GAINS) or null
template <bool GAINS>
__global__ __launch_bounds__(UND_BLOCK) void undistort_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const TrkIntr cam,
                                                              const UndPinhole pin, int W, int H, int Wo, int Ho, uint32_t border,
                                                              const int64_t *__restrict__ gains)
{
    const int b = blockIdx.z; // uniform
    const int lx = threadIdx.x % UND_LANES_X, ly = threadIdx.x / UND_LANES_X;
    const int j = blockIdx.y * UND_TILE_H + ly, i0 = blockIdx.x * UND_TILE_W + lx * UND_PIXELS;
    if (j >= Ho || i0 >= Wo) return; // nothing below synchronises the workgroup
    const uint8_t *__restrict__ tb = src + 3 * (int64_t)b * ((int64_t)W * H);
    int64_t g[6] = {0, 0, 0, 0, 0, 0};
    if (GAINS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = gains[6 * (int64_t)b + k]; // uniform address: scalar loads
    }
    const int npx = min(UND_PIXELS, Wo - i0);
    uint32_t px[UND_PIXELS];
#pragma unroll
    for (int q = 0; q < UND_PIXELS; ++q) {
        px[q] = 0u;
        if (q < npx)
            und_pixel(cam, pin, W, H, i0 + q, j, border, GAINS ? g : nullptr,
                      [&](int y, int x) { return photo_texel_of(tb + 3 * ((int64_t)y * W + x)); }, px[q]);
    }
    uint32_t d[3];
    und_pack(px, d);
    uint8_t *__restrict__ o = dst + 3 * ((int64_t)b * ((int64_t)Wo * Ho) + (int64_t)j * Wo + i0);
    // byte q of the lane's run
    const auto byte_of = [&](int q) { return (uint8_t)(((q < 4 ? d[0] : (q < 8 ? d[1] : d[2])) >> (8 * (q & 3))) & 255u); };
    if (npx < UND_PIXELS) { // the image's right edge: 3, 6 or 9 bytes
        for (int q = 0; q < 3 * npx; ++q) o[q] = byte_of(q);
        return;
    }
    const int a = (int)((4u - (unsigned)((uintptr_t)o & 3u)) & 3u); // bytes before the first aligned dword
    if (a == 0) {
        uint32_t *__restrict__ o4 = (uint32_t *)o;
        o4[0] = d[0]; o4[1] = d[1]; o4[2] = d[2];
        return;
    }
    // head a bytes, two aligned dwords (bytes a .. a + 7 of the run), tail 4 - a bytes
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (q < a) o[q] = byte_of(q);
    const int sh = 8 * a;
    uint32_t *__restrict__ o4 = (uint32_t *)(o + a);
    o4[0] = (d[0] >> sh) | (d[1] << (32 - sh));
    o4[1] = (d[1] >> sh) | (d[2] << (32 - sh));
#pragma unroll
    for (int q = 9; q < 12; ++q)
        if (q >= a + 8) o[q] = byte_of(q);
}

// uv [Ho][Wo][2] (NaN where invalid) and mask [Ho][Wo] (255 valid, 0 not); either may be null
__global__ __launch_bounds__(256) void undistort_map_kernel(const TrkIntr cam, const UndPinhole pin, int W, int H, int Wo, int Ho,
                                                            double *__restrict__ uv, uint8_t *__restrict__ mask)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)Wo * Ho) return;
    const int j = (int)(q / Wo), i = (int)(q - (int64_t)j * Wo);
    double u, v;
    const bool ok = und_locate(cam, pin, W, H, i, j, u, v);
    if (uv) { uv[2 * q] = ok ? u : (double)NAN; uv[2 * q + 1] = ok ? v : (double)NAN; }
    if (mask) mask[q] = ok ? (uint8_t)255 : (uint8_t)0;
}

// the map kernel into host arrays, either of which may be null
int32_t run_map(lvba_undistort_s *h, double *uv, uint8_t *mask)
{
    HIPCHK(hipSetDevice(h->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    const int64_t npix = (int64_t)h->out_width * h->out_height;
    DevArr<double> d_uv(s);
    DevArr<uint8_t> d_mask(s);
    if (uv) HIPCHK(d_uv.alloc(2 * (size_t)npix));
    if (mask) HIPCHK(d_mask.alloc((size_t)npix));
    undistort_map_kernel<<<grid_for(npix, 256), 256, 0, s>>>(h->cam, h->pin, h->width, h->height, h->out_width, h->out_height,
                                                              uv ? (double *)d_uv : nullptr, mask ? (uint8_t *)d_mask : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (uv) HIPCHK(d_uv.download(uv, 2 * (size_t)npix));
    if (mask) HIPCHK(d_mask.download(mask, (size_t)npix));
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_undistort_default_opts(lvba_undistort_opts *o)
{
    if (!o) return;
    *o = lvba_undistort_opts{}; // fx 0: the source's pinhole; sizes 0: the source's; border 0
    o->max_batch_images = 64;   // the kernel is saturated long before; the stage's device memory stays small beside the map's
}

extern "C" int32_t lvba_undistort_tile(int32_t *pixels_per_lane, int32_t *tile_width, int32_t *tile_height)
{
    if (!pixels_per_lane || !tile_width || !tile_height) return lvba_fail(LVBA_ERR_ARG, "null output");
    *pixels_per_lane = UND_PIXELS; *tile_width = UND_TILE_W; *tile_height = UND_TILE_H;
    return LVBA_OK;
}

extern "C" int32_t lvba_undistort_create(int32_t device, int32_t width, int32_t height, const double intr[8], const lvba_undistort_opts *opts,
                                         lvba_undistort_t *out)
{
    if (!out) return lvba_fail(LVBA_ERR_ARG, "null output");
    if (!intr) return lvba_fail(LVBA_ERR_ARG, "null intrinsics");
    if (width < 2 || height < 2) return lvba_fail(LVBA_ERR_ARG, "image size %d x %d (both must be >= 2)", width, height);
    TRY(check_intrinsics_finite(intr));
    TRY(check_focal_lengths(intr));
    lvba_undistort_opts o;
    lvba_undistort_default_opts(&o);
    if (opts) o = *opts;
    if (o.fx == 0.0) { o.fx = intr[0]; o.fy = intr[1]; o.cx = intr[2]; o.cy = intr[3]; }
    if (o.out_width == 0) o.out_width = width;
    if (o.out_height == 0) o.out_height = height;
    if (!(std::isfinite(o.fx) && std::isfinite(o.fy) && std::isfinite(o.cx) && std::isfinite(o.cy)) || !(o.fx > 0.0 && o.fy > 0.0))
        return lvba_fail(LVBA_ERR_ARG, "target pinhole %g %g %g %g (finite, focal lengths > 0; fx = 0: the source's)", o.fx, o.fy, o.cx, o.cy);
    if (o.out_width < 2 || o.out_height < 2 || o.border < 0 || o.border > 255 || o.max_batch_images < 0)
        return lvba_fail(LVBA_ERR_ARG, "options: target size %d x %d (0, or both >= 2), border %d (0 .. 255), max_batch_images %d (>= 0)",
                         o.out_width, o.out_height, o.border, o.max_batch_images);
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_undistort_s *h = new (std::nothrow) lvba_undistort_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    struct Guard { lvba_undistort_s *h; ~Guard() { delete h; } } guard{h};
    h->device = device; h->width = width; h->height = height; h->out_width = o.out_width; h->out_height = o.out_height;
    h->cam = trk_intr_of(intr);
    h->pin = UndPinhole{o.fx, o.fy, o.cx, o.cy};
    h->border = (uint32_t)o.border;
    h->max_batch = o.max_batch_images;
    std::vector<uint8_t> mask((size_t)o.out_width * (size_t)o.out_height);
    TRY(run_map(h, nullptr, mask.data()));
    for (const uint8_t m : mask) h->n_valid += m ? 1 : 0;
    *out = h;
    guard.h = nullptr;
    return LVBA_OK;
}

extern "C" int32_t lvba_undistort_info(lvba_undistort_t h, int32_t *out_width, int32_t *out_height, double pinhole[4], int64_t *n_valid)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (out_width) *out_width = h->out_width;
    if (out_height) *out_height = h->out_height;
    if (pinhole) { pinhole[0] = h->pin.fx; pinhole[1] = h->pin.fy; pinhole[2] = h->pin.cx; pinhole[3] = h->pin.cy; }
    if (n_valid) *n_valid = h->n_valid;
    return LVBA_OK;
}

extern "C" int32_t lvba_undistort_images(lvba_undistort_t h, int32_t n, const uint8_t *bgr, const int64_t *gains, uint8_t *bgr_out)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (n < 0) return lvba_fail(LVBA_ERR_ARG, "%d images (>= 0)", n);
    if (n == 0) return LVBA_OK;
    if (!bgr || !bgr_out) return lvba_fail(LVBA_ERR_ARG, "null images or output");
    if (gains && !expo_gains_ok(gains, 3 * (int64_t)n))
        return lvba_fail(LVBA_ERR_ARG, "gains: A outside [2^14, 2^18] or |B| above 2^16 * 65280");
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)h->width * h->height, opix = (int64_t)h->out_width * h->out_height;
    // the batch: the uploaded bytes and the undistorted bytes of B images
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(0.4 * ((double)free_b + (double)DevicePool::get().cached_bytes()), 8.0 * (1 << 30));
    int64_t B = std::max<int64_t>(1, (int64_t)(budget / (3.0 * (double)(npix + opix))));
    if (h->max_batch > 0) B = std::min<int64_t>(B, h->max_batch);
    B = std::min<int64_t>(std::min<int64_t>(B, n), UND_MAX_BATCH);
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<4> ev;
    DevArr<uint8_t> d_src(s), d_dst(s); DevArr<int64_t> d_g(s);
    HIPCHK(d_src.alloc(3 * (size_t)npix * (size_t)B));
    HIPCHK(d_dst.alloc(3 * (size_t)opix * (size_t)B));
    if (gains) HIPCHK(d_g.alloc(6 * (size_t)B));
    const unsigned gx = grid_for(h->out_width, UND_TILE_W), gy = grid_for(h->out_height, UND_TILE_H);
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int nb = (int)std::min<int64_t>(B, n - b0);
        ev.rec(0, s);
        HIPCHK(hipMemcpyAsync(d_src, bgr + 3 * npix * b0, 3 * (size_t)npix * nb, hipMemcpyHostToDevice, s));
        if (gains) HIPCHK(hipMemcpyAsync(d_g, gains + 6 * b0, d_g.bytes(6 * (size_t)nb), hipMemcpyHostToDevice, s));
        ev.rec(1, s);
        const auto kernel = gains ? undistort_kernel<true> : undistort_kernel<false>;
        kernel<<<dim3(gx, gy, (unsigned)nb), UND_BLOCK, 0, s>>>(d_src, d_dst, h->cam, h->pin, h->width, h->height, h->out_width, h->out_height,
                                                               h->border, gains ? (const int64_t *)d_g : nullptr);
        HIPCHK(hipGetLastError());
        ev.rec(2, s);
        HIPCHK(hipMemcpyAsync(bgr_out + 3 * opix * b0, d_dst, 3 * (size_t)opix * nb, hipMemcpyDeviceToHost, s));
        ev.rec(3, s);
        HIPCHK(hipStreamSynchronize(s));
        h->ms[0] += ev.ms(0, 1); h->ms[1] += ev.ms(1, 2); h->ms[2] += ev.ms(2, 3);
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_undistort_map(lvba_undistort_t h, double *uv, uint8_t *mask)
{
    if (!h) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (!uv && !mask) return LVBA_OK;
    return run_map(h, uv, mask);
}

extern "C" int32_t lvba_undistort_profile(lvba_undistort_t h, double ms[3])
{
    if (!h || !ms) return lvba_fail(LVBA_ERR_ARG, "null handle or output");
    ms[0] = h->ms[0]; ms[1] = h->ms[1]; ms[2] = h->ms[2];
    return LVBA_OK;
}

extern "C" void lvba_undistort_free(lvba_undistort_t h)
{
    delete h;
}
