// colorize.hip -- the LiDAR map coloured from the camera images, on the device.
//
// Replaces, of the reference (paths relative to its source tree):
//   LvbaSystem::VisualizeOptComparison   src/lvba_system.cpp:1932-2144   per image: every point of every scan within +-0.5 s
//                                        in the world frame (float), projected through the distortion model, a depth buffer
//                                        (zc + 1e-6f < zbuf, zbuf = (float)zc) keeps one point per pixel, which takes the
//                                        pixel's BGR; survivors in row-major pixel order, images concatenated, then
//   down_sampling_voxel2                 include/BALM/tools.hpp:300-359  the first point at minimum distance to its leaf
//                                        centre per leaf voxel
// The per-point rules are colorize_device.h (also compiled for the host by the tests).
//
// Device design: a handle holds the float world points of one pose set.  Images come in
// batches sized by free memory: one lane per (image, window point) projects and emits the key (image in batch, pixel) with
// its work index -- the work index grows with the point order inside an image --; a stable radix sort on the key bits groups
// each pixel's points in point order, and one lane per pixel segment walks the reference's depth-buffer rule literally (no
// pruning: with the epsilon and the float store, points that cannot win can still decide which point does).  Kept pixels are
// compacted in (image, row-major pixel) order, i.e. the reference's merge order, and take their colour.
// Thinning: the first minimum of d2 in merged order per leaf key is the lexicographic minimum of (d2, merged position), an
// associative reduction, so every batch is appended to the running key-sorted set and the union is reduced again: memory stays
// bounded by the map, and the result does not depend on the batch size.  Output order: by leaf key (x, y, z), as the window
// stage's down-sampling (window_ba.hip); the reference's is unordered_map order (unspecified).  Without thinning: merged order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "tracks_device.h"
#include "colorize_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr uint32_t COL_SENT = 0xFFFFFFFFu; // key of a work item whose point is skipped (sorts after every pixel)

} // namespace

struct lvba_colorize_s {
    int device = 0;
    int n_frames = 0, width = 0, height = 0;
    TrkIntr cam{};
    double half = 0.5, leaf = 0.01;
    int32_t max_batch = 0;
    bool thin = true;
    std::vector<int64_t> frame_off;
    std::vector<double> scan_times;
    // handle-owned device arrays (no stream: every call has drained its own before it returned)
    DevArr<float> world; // [P][3]
    int64_t n_merged = 0; // points emitted so far (merged position of the next one)
    // the running set: n points (key-sorted and one per leaf when thinning, else in merged order), capacity cap
    int64_t n = 0, cap = 0;
    DevArr<float> xyz;   // [cap][3]
    DevArr<uint8_t> rgb; // [cap][3]
    DevArr<uint64_t> key;
    DevArr<double> d2;
    DevArr<int64_t> pos;
    double prof[6] = {0, 0, 0, 0, 0, 0}; // upload, projection, sort, walk, compaction, thinning (ms, accumulated)
    ~lvba_colorize_s()
    {
        (void)hipSetDevice(device);
        world.reset(); xyz.reset(); rgb.reset(); key.reset(); d2.reset(); pos.reset();
    }
};

namespace {

// col_world_kernel: colorize_device.h (shared with map_quality.hip)

struct BatchImage {
    int64_t p0, np, w0; // first world point, points in the window, first work item
};

// one lane per (image b of the batch, point of its window)
__global__ void col_project_kernel(const BatchImage *__restrict__ tab, const float *__restrict__ world, const double *__restrict__ Rcw,
                                   const double *__restrict__ tcw, TrkIntr cam, int W, int H, uint32_t *__restrict__ key,
                                   uint32_t *__restrict__ val, double *__restrict__ zc)
{
    const int b = blockIdx.y;
    const BatchImage t = tab[b];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.np) return;
    const int64_t p = t.p0 + i, j = t.w0 + i;
    const float pw[3] = {world[3 * p], world[3 * p + 1], world[3 * p + 2]};
    int64_t pix = 0;
    double z = 0.0;
    const bool ok = col_project(cam, Rcw + 9 * b, tcw + 3 * b, pw, W, H, pix, z);
    key[j] = ok ? (uint32_t)((int64_t)b * W * H + pix) : COL_SENT;
    val[j] = (uint32_t)j;
    zc[j] = z;
}

// one lane per sorted position; the first of a pixel's run walks the run (colorize_device.h col_walk)
__global__ void col_walk_kernel(int64_t M, const uint32_t *__restrict__ key_s, const uint32_t *__restrict__ val_s,
                                const double *__restrict__ zc, uint32_t *__restrict__ flag, uint32_t *__restrict__ win)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const uint32_t k = key_s[i];
    if (k == COL_SENT || (i > 0 && key_s[i - 1] == k)) { flag[i] = 0u; return; }
    int64_t e = i + 1;
    while (e < M && key_s[e] == k) ++e;
    int64_t w;
    const bool kept = col_walk(e - i, [&](int64_t q) { return zc[val_s[i + q]]; }, w);
    flag[i] = kept ? 1u : 0u;
    win[i] = kept ? val_s[i + w] : 0u;
}

// kept pixel -> the running set's slot R + rank: position, colour, leaf key and d2
__global__ void col_emit_kernel(int64_t M, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                const uint32_t *__restrict__ key_s, const uint32_t *__restrict__ win, const BatchImage *__restrict__ tab,
                                int64_t npix, const float *__restrict__ world, const uint8_t *__restrict__ bgr, double leaf, int thin,
                                int64_t R, int64_t pos0, float *__restrict__ xyz, uint8_t *__restrict__ rgb, uint64_t *__restrict__ okey,
                                double *__restrict__ od2, int64_t *__restrict__ opos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || !flag[i]) return;
    const int64_t o = R + excl[i];
    const int64_t b = key_s[i] / npix, pix = key_s[i] % npix;
    const BatchImage t = tab[b];
    const int64_t p = t.p0 + ((int64_t)win[i] - t.w0);
    const float q[3] = {world[3 * p], world[3 * p + 1], world[3 * p + 2]};
    xyz[3 * o] = q[0]; xyz[3 * o + 1] = q[1]; xyz[3 * o + 2] = q[2];
    const uint8_t *c = bgr + 3 * (b * npix + pix);
    rgb[3 * o] = c[2]; rgb[3 * o + 1] = c[1]; rgb[3 * o + 2] = c[0];
    opos[o] = pos0 + excl[i];
    if (thin) {
        int64_t k[3];
        double dd;
        leaf_key_of(q, leaf, k, dd); // in range: every finite world point was checked at creation
        okey[o] = pack_key(k);
        od2[o] = dd;
    }
}

__global__ void col_iota_kernel(int64_t n, uint32_t *__restrict__ v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}
// run leader of a leaf key: the lexicographic minimum of (d2, merged position) = the first minimum of d2 in merged order
__global__ void col_pick_kernel(int64_t n, const uint64_t *__restrict__ key_s, const uint32_t *__restrict__ idx_s,
                                const double *__restrict__ d2, const int64_t *__restrict__ pos, uint32_t *__restrict__ flag,
                                uint32_t *__restrict__ pick)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key_s[i];
    if (i > 0 && key_s[i - 1] == k) { flag[i] = 0u; return; }
    uint32_t best = idx_s[i];
    double bd = d2[best];
    int64_t bp = pos[best];
    for (int64_t j = i + 1; j < n && key_s[j] == k; ++j) {
        const uint32_t c = idx_s[j];
        const double d = d2[c];
        const int64_t pc = pos[c];
        if (d < bd || (d == bd && pc < bp)) { bd = d; bp = pc; best = c; }
    }
    flag[i] = 1u;
    pick[i] = best;
}
__global__ void col_gather_kernel(int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                  const uint32_t *__restrict__ pick, const float *__restrict__ xyz, const uint8_t *__restrict__ rgb,
                                  const uint64_t *__restrict__ key, const double *__restrict__ d2, const int64_t *__restrict__ pos,
                                  float *__restrict__ xyz2, uint8_t *__restrict__ rgb2, uint64_t *__restrict__ key2,
                                  double *__restrict__ d22, int64_t *__restrict__ pos2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t s = pick[i], o = excl[i];
    for (int c = 0; c < 3; ++c) { xyz2[3 * o + c] = xyz[3 * s + c]; rgb2[3 * o + c] = rgb[3 * s + c]; }
    key2[o] = key[s]; d22[o] = d2[s]; pos2[o] = pos[s];
}

// the running set's five arrays for `cap` points, not yet the handle's; adopt() hands them over once the stream has drained, what is
// not adopted drains the stream and goes back to the pool
struct RunningSet {
    DevArr<float> xyz; DevArr<uint8_t> rgb; DevArr<uint64_t> key; DevArr<double> d2; DevArr<int64_t> pos;
    explicit RunningSet(hipStream_t s) : xyz(s), rgb(s), key(s), d2(s), pos(s) {}
    int32_t alloc(size_t cap)
    {
        hipError_t e = xyz.alloc(3 * cap);
        if (e == hipSuccess) e = rgb.alloc(3 * cap);
        if (e == hipSuccess) e = key.alloc(cap);
        if (e == hipSuccess) e = d2.alloc(cap);
        if (e == hipSuccess) e = pos.alloc(cap);
        return e == hipSuccess ? LVBA_OK : lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "colour map: %s", hipGetErrorString(e));
    }
    void adopt(lvba_colorize_s *h, int64_t cap)
    {
        h->xyz.reset(xyz.release()); h->rgb.reset(rgb.release()); h->key.reset(key.release()); h->d2.reset(d2.release()); h->pos.reset(pos.release());
        h->cap = cap;
    }
};

// grow the running set to hold `need` points, keeping its first h->n
int32_t ensure_capacity(lvba_colorize_s *h, int64_t need, hipStream_t s)
{
    if (need <= h->cap) return LVBA_OK;
    const int64_t cap = std::max<int64_t>(need, h->cap + h->cap / 2);
    RunningSet a(s);
    TRY(a.alloc((size_t)cap));
    const size_t n = (size_t)h->n;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(a.xyz, h->xyz, a.xyz.bytes(3 * n), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(a.rgb, h->rgb, a.rgb.bytes(3 * n), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(a.key, h->key, a.key.bytes(n), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(a.d2, h->d2, a.d2.bytes(n), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(a.pos, h->pos, a.pos.bytes(n), hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    a.adopt(h, cap);
    return LVBA_OK;
}

// reduce the running set [0, h->n) to one point per leaf key, sorted by key
int32_t thin_running(lvba_colorize_s *h, hipStream_t s)
{
    const int64_t n = h->n;
    if (n == 0) return LVBA_OK;
    DevArr<uint32_t> idx(s);
    DevArr<uint64_t> key_s(s);
    DevArr<uint32_t> idx_s(s), flag(s), excl(s), pick(s);
    HIPCHK(idx.alloc((size_t)n)); HIPCHK(key_s.alloc((size_t)n)); HIPCHK(idx_s.alloc((size_t)n));
    HIPCHK(flag.alloc((size_t)n)); HIPCHK(excl.alloc((size_t)n)); HIPCHK(pick.alloc((size_t)n));
    col_iota_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, idx);
    HIPCHK(hipGetLastError());
    TRY(sort_pairs<uint64_t>(s, h->key, key_s, idx, idx_s, (size_t)n, 63));
    col_pick_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, key_s, idx_s, h->d2, h->pos, flag, pick);
    HIPCHK(hipGetLastError());
    int64_t N = 0;
    TRY(count_flags(s, flag, excl, (size_t)n, &N));
    RunningSet a(s);
    const int64_t cap = std::max<int64_t>(N, 1);
    TRY(a.alloc((size_t)cap));
    col_gather_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, flag, excl, pick, h->xyz, h->rgb, h->key, h->d2, h->pos, a.xyz, a.rgb,
                                                       a.key, a.d2, a.pos);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    a.adopt(h, cap);
    h->n = N;
    return LVBA_OK;
}

// one batch: images [b0, b1) of the call, all with a non-empty window (tab[] filled by the caller)
int32_t run_batch(lvba_colorize_s *h, hipStream_t s, const std::vector<BatchImage> &tab, const std::vector<int32_t> &img_of,
                  const double *Rcw, const double *tcw, const uint8_t *bgr, int64_t M)
{
    const int B = (int)tab.size();
    const int64_t npix = (int64_t)h->width * h->height;
    EventTimer<7> ev;
    ev.rec(0, s);
    DevArr<BatchImage> d_tab(s);
    DevArr<double> d_R(s), d_t(s);
    DevArr<uint8_t> d_img(s);
    DevArr<uint32_t> key(s), val(s), key_s(s), val_s(s);
    DevArr<double> zc(s);
    DevArr<uint32_t> flag(s), excl(s), win(s);
    HIPCHK(d_tab.alloc((size_t)B)); HIPCHK(d_R.alloc(9 * (size_t)B)); HIPCHK(d_t.alloc(3 * (size_t)B));
    HIPCHK(d_img.alloc(3 * (size_t)npix * B));
    std::vector<double> R(9 * (size_t)B), t(3 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const int64_t k = img_of[b];
        std::copy(Rcw + 9 * k, Rcw + 9 * k + 9, R.begin() + 9 * b);
        std::copy(tcw + 3 * k, tcw + 3 * k + 3, t.begin() + 3 * b);
        HIPCHK(hipMemcpyAsync(d_img + 3 * npix * b, bgr + 3 * npix * k, 3 * (size_t)npix, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), d_tab.bytes(B), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_R, R.data(), d_R.bytes(R.size()), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_t, t.data(), d_t.bytes(t.size()), hipMemcpyHostToDevice, s));
    ev.rec(1, s);
    HIPCHK(key.alloc((size_t)M)); HIPCHK(val.alloc((size_t)M)); HIPCHK(key_s.alloc((size_t)M));
    HIPCHK(val_s.alloc((size_t)M)); HIPCHK(zc.alloc((size_t)M)); HIPCHK(flag.alloc((size_t)M));
    HIPCHK(excl.alloc((size_t)M)); HIPCHK(win.alloc((size_t)M));
    int64_t max_np = 0;
    for (const auto &x : tab) max_np = std::max(max_np, x.np);
    col_project_kernel<<<dim3(grid_for(max_np, 256), B), 256, 0, s>>>(d_tab, h->world, d_R, d_t, h->cam, h->width, h->height, key,
                                                                      val, zc);
    HIPCHK(hipGetLastError());
    ev.rec(2, s);
    unsigned bits = 1; // keys < B * npix, and the sentinel's low bits (all ones) above every one of them
    while (bits < 32 && ((uint64_t)1 << bits) - 1 < (uint64_t)B * npix) ++bits;
    TRY(sort_pairs<uint32_t>(s, key, key_s, val, val_s, (size_t)M, bits));
    ev.rec(3, s);
    col_walk_kernel<<<grid_for(M, 256), 256, 0, s>>>(M, key_s, val_s, zc, flag, win);
    HIPCHK(hipGetLastError());
    ev.rec(4, s);
    int64_t S = 0;
    TRY(count_flags(s, flag, excl, (size_t)M, &S));
    if (S > 0) {
        TRY(ensure_capacity(h, h->n + S, s));
        col_emit_kernel<<<grid_for(M, 256), 256, 0, s>>>(M, flag, excl, key_s, win, d_tab, npix, h->world, d_img, h->leaf,
                                                         h->thin ? 1 : 0, h->n, h->n_merged, h->xyz, h->rgb, h->key, h->d2, h->pos);
        HIPCHK(hipGetLastError());
    }
    ev.rec(5, s);
    h->n += S;
    h->n_merged += S;
    if (h->thin && S > 0) TRY(thin_running(h, s));
    ev.rec(6, s);
    HIPCHK(hipStreamSynchronize(s));
    for (int p = 0; p < 6; ++p) h->prof[p] += ev.ms(p, p + 1);
    return LVBA_OK;
}

bool all_finite(const double *v, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

} // namespace

extern "C" void lvba_colorize_default_opts(lvba_colorize_opts *o)
{
    if (!o) return;
    o->half_window_s = 0.5;     // src/lvba_system.cpp:1974
    o->leaf_size = 0.01;        // config: filter_size_points3D
    o->max_batch_images = 0;    // by free memory
    o->reserved = 0;
}

extern "C" int32_t lvba_colorize_create(lvba_scans_t sc, const double *scan_poses, const double *scan_times, const double intr[8],
                                        int32_t width, int32_t height, const lvba_colorize_opts *opts, lvba_colorize_t *out)
{
    if (out) *out = nullptr;
    if (!sc || !scan_poses || !scan_times || !intr || !out) return lvba_fail(LVBA_ERR_ARG, "null argument");
    if (width < 2 || height < 2) return lvba_fail(LVBA_ERR_ARG, "image size %d x %d (both must be >= 2)", width, height);
    lvba_colorize_opts o;
    lvba_colorize_default_opts(&o);
    if (opts) o = *opts;
    if (!(o.half_window_s >= 0) || !std::isfinite(o.half_window_s) || !std::isfinite(o.leaf_size) || o.max_batch_images < 0)
        return lvba_fail(LVBA_ERR_ARG, "options: half_window_s %g, leaf_size %g, max_batch_images %d", o.half_window_s, o.leaf_size,
                         o.max_batch_images);
    if ((int64_t)width * height * 3 > ((int64_t)1 << 31)) return lvba_fail(LVBA_ERR_ARG, "image size %d x %d too large", width, height);
    const int nf = sc->n_frames;
    if (!all_finite(scan_poses, 12 * (int64_t)nf) || !all_finite(scan_times, nf) || !all_finite(intr, 8))
        return lvba_fail(LVBA_ERR_ARG, "non-finite scan pose, scan time or intrinsic");
    for (int f = 1; f < nf; ++f)
        if (scan_times[f] < scan_times[f - 1]) return lvba_fail(LVBA_ERR_ARG, "scan times not ascending at scan %d", f);
    HIPCHK(hipSetDevice(sc->device));
    lvba_colorize_s *h = new (std::nothrow) lvba_colorize_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    struct Guard { lvba_colorize_s *h; ~Guard() { delete h; } } guard{h};
    h->device = sc->device; h->n_frames = nf; h->width = width; h->height = height;
    h->cam = trk_intr_of(intr);
    h->half = o.half_window_s; h->leaf = o.leaf_size; h->max_batch = o.max_batch_images;
    h->thin = !(o.leaf_size < 0.001); // down_sampling_voxel2: a leaf below 1 mm means no thinning
    h->frame_off.assign(sc->frame_off.begin(), sc->frame_off.begin() + nf + 1);
    h->scan_times.assign(scan_times, scan_times + nf);
    const int64_t P = h->frame_off[nf];
    if (P >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_ARG, "%lld points (at most 2^32 - 1)", (long long)P);
    HIPCHK(h->world.alloc(3 * (size_t)std::max<int64_t>(P, 1)));
    if (P > 0) {
        ScopedStream sg;
        HIPCHK(sg.acquire());
        const hipStream_t s = sg.s;
        DevArr<double> d_poses(s);
        DevArr<int> d_err(s);
        HIPCHK(d_poses.alloc(12 * (size_t)nf)); HIPCHK(d_err.alloc(1));
        HIPCHK(hipMemcpyAsync(d_poses, scan_poses, d_poses.bytes(12 * (size_t)nf), hipMemcpyHostToDevice, s));
        HIPCHK(d_err.zero_async(1));
        col_world_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, sc->d_pts, sc->d_frame_off, nf, d_poses, h->leaf, h->thin ? 1 : 0,
                                                          h->world, d_err);
        HIPCHK(hipGetLastError());
        int err = 0;
        HIPCHK(hipMemcpyAsync(&err, d_err, d_err.bytes(1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (err) return lvba_fail(LVBA_ERR_ARG, "a world point lies outside +-2^20 leaves of %g m", h->leaf);
    }
    *out = h;
    guard.h = nullptr;
    return LVBA_OK;
}

extern "C" int32_t lvba_colorize_add_images(lvba_colorize_t h, int32_t n, const double *image_times, const double *Rcw,
                                            const double *tcw, const uint8_t *bgr)
{
    if (!h || n < 0 || (n > 0 && (!image_times || !Rcw || !tcw || !bgr))) return lvba_fail(LVBA_ERR_ARG, "null argument or n < 0");
    if (n == 0) return LVBA_OK;
    if (!all_finite(image_times, n) || !all_finite(Rcw, 9 * (int64_t)n) || !all_finite(tcw, 3 * (int64_t)n))
        return lvba_fail(LVBA_ERR_ARG, "non-finite image time or camera pose");
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)h->width * h->height;
    // batch budget: ~40 bytes per work item (keys, values, sorted copies, depth, flags; the sort's scratch) + the images
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(0.4 * (double)free_b, 8.0 * (1 << 30));
    const int64_t max_b = std::max<int64_t>(1, std::min<int64_t>(h->max_batch > 0 ? h->max_batch : INT32_MAX, (((int64_t)1 << 31) - 1) / npix));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    std::vector<BatchImage> tab;
    std::vector<int32_t> img_of;
    int64_t M = 0;
    for (int k = 0; k <= n; ++k) {
        BatchImage bi{0, 0, 0};
        if (k < n) {
            int lo, hi;
            col_window_range(h->scan_times.data(), h->n_frames, image_times[k], h->half, lo, hi);
            if (hi <= lo || h->frame_off[hi] == h->frame_off[lo]) continue; // :1991-1996: no LiDAR in the window
            bi.p0 = h->frame_off[lo];
            bi.np = h->frame_off[hi] - bi.p0;
        }
        const bool fits = k < n && (int64_t)tab.size() < max_b && M + bi.np < ((int64_t)1 << 32) - 1 &&
                          40.0 * (double)(M + bi.np) + 3.0 * (double)npix * (double)(tab.size() + 1) <= budget;
        if (!tab.empty() && !fits) {
            TRY(run_batch(h, s, tab, img_of, Rcw, tcw, bgr, M));
            tab.clear(); img_of.clear(); M = 0;
        }
        if (k == n) break;
        bi.w0 = M;
        tab.push_back(bi);
        img_of.push_back(k);
        M += bi.np;
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_colorize_count(lvba_colorize_t h, int64_t *n_points)
{
    if (!h || !n_points) return lvba_fail(LVBA_ERR_ARG, "null argument");
    *n_points = h->n;
    return LVBA_OK;
}

extern "C" int32_t lvba_colorize_download(lvba_colorize_t h, float *xyz, uint8_t *rgb)
{
    if (!h || (h->n > 0 && (!xyz || !rgb))) return lvba_fail(LVBA_ERR_ARG, "null argument");
    if (h->n == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(xyz, h->xyz, h->xyz.bytes(3 * (size_t)h->n), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rgb, h->rgb, h->rgb.bytes(3 * (size_t)h->n), hipMemcpyDeviceToHost));
    return LVBA_OK;
}

extern "C" int32_t lvba_colorize_profile(lvba_colorize_t h, double ms[6])
{
    if (!h || !ms) return lvba_fail(LVBA_ERR_ARG, "null argument");
    for (int p = 0; p < 6; ++p) ms[p] = h->prof[p];
    return LVBA_OK;
}

extern "C" void lvba_colorize_destroy(lvba_colorize_t h)
{
    delete h;
}
