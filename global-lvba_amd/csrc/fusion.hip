// fusion.hip -- LiDAR-assisted landmark initialisation on the device (the step before the
// visual solve): depth images rendered from the refined LiDAR map, then one lane per feature track forms the depth-fused and
// the triangulated candidate and picks one.
//
// Replaces, of the reference (paths relative to /root/reference):
//   LvbaSystem::buildGridMapFromOptimized   src/lvba_system.cpp:1266-1338   every scan point in the world frame, hashed into
//                                           0.5 m voxels (float key quotient, -1 if negative); per image: the voxels touched
//                                           by the scans within +-0.5 s of it
//   LvbaSystem::generateDepthWithVoxel      src/lvba_system.cpp:835-919     z-buffer over ALL map points of those voxels:
//                                           pixel (int)u, (int)v; Z < 1e-3 skipped; the smallest (float)Z wins
//   LvbaSystem::BuildTracksAndFuse3D        src/lvba_system.cpp:1016-1225   per BFS component: depth-fused candidate (bilinear
//                                           depth, back-projection through the distortion model, 0.12 m consistency with the
//                                           first valid observation, first observation per image, greedy view-angle filter,
//                                           mean reprojection error), triangulation candidate (DLT seed, the same filter, DLT
//                                           again), selection by mean reprojection error
//   fetchDepthBilinear, backProjectPixelDepthDistorted, camToWorld          include/utils.hpp:235-284
// The reference walks std::unordered_map<int,int> (image -> observation) wherever it iterates over a track's images, an
// unspecified order; here images are visited in the order of their first occurrence in the component.
//
// Device design: the grid map is one radix sort of (voxel key, point) pairs; an image's voxel set is a mark array filled by
// the points of the scans in its time window (a contiguous range of the scan set); marked voxels are expanded to point
// work items by a scan, one thread per map point projects and does one atomicMin on the float bits of the depth image
// (positive floats order like their bit patterns, so the smallest (float)Z wins whatever the order, as in the reference).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "segments.h"
#include "image_set.h"
#include "tracks_device.h"
#include "fusion_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

__global__ void gm_world_kernel(int64_t P, const float *__restrict__ pts, const int64_t *__restrict__ frame_off, int n_frames,
                                const double *__restrict__ poses, double vox, double *__restrict__ world,
                                uint64_t *__restrict__ key, uint32_t *__restrict__ idx, int *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    double pw[3];
    pose_apply(poses + 12 * (int64_t)frame_of_point(frame_off, n_frames, i), pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pw);
    int64_t k[3];
    if (!root_key_of(pw, vox, k)) { *err = 1; k[0] = k[1] = k[2] = 0; }
    world[3 * i] = pw[0]; world[3 * i + 1] = pw[1]; world[3 * i + 2] = pw[2];
    key[i] = pack_key(k);
    idx[i] = (uint32_t)i;
}
__global__ void gm_heads_kernel(int64_t P, const uint64_t *__restrict__ key_s, uint32_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) head[i] = (i == 0 || key_s[i] != key_s[i - 1]) ? 1u : 0u;
}
// vidx_s = inclusive scan of head - 1: voxel of every sorted position; voff[v] = first sorted position of voxel v
__global__ void gm_tables_kernel(int64_t P, const uint32_t *__restrict__ head, const uint32_t *__restrict__ incl,
                                 const uint32_t *__restrict__ order, uint32_t *__restrict__ vox_of_point,
                                 int64_t *__restrict__ voff, int64_t V)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t v = incl[i] - 1;
    vox_of_point[order[i]] = v;
    if (head[i]) voff[v] = i;
    if (i == P - 1) voff[V] = P;
}
__global__ void gm_mark_kernel(int64_t n, const uint32_t *__restrict__ vox_of_point, uint32_t *__restrict__ mark)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mark[vox_of_point[i]] = 1u;
}
__global__ void gm_count_kernel(int64_t V, const uint32_t *__restrict__ mark, const int64_t *__restrict__ voff,
                                int64_t *__restrict__ cnt)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) cnt[v] = mark[v] ? voff[v + 1] - voff[v] : 0;
    if (v == V) cnt[V] = 0;
}
// one thread per map point of the image's voxel set (generateDepthWithVoxel's inner loop, :886-905)
__global__ void gm_render_kernel(int64_t M, int64_t V, const int64_t *__restrict__ start /*[V+1] exclusive scan of cnt*/,
                                 const int64_t *__restrict__ voff, const uint32_t *__restrict__ order,
                                 const double *__restrict__ world, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                                 TrkIntr cam, int width, int height, unsigned int *__restrict__ depth_bits)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const int64_t lo = segment_of(start, V, j);
    const int64_t pos = voff[lo] + (j - start[lo]);
    const double *pw = world + 3 * (int64_t)order[pos];
    const double X0 = Rcw[0] * pw[0] + Rcw[1] * pw[1] + Rcw[2] * pw[2] + tcw[0];
    const double X1 = Rcw[3] * pw[0] + Rcw[4] * pw[1] + Rcw[5] * pw[2] + tcw[1];
    const double Z = Rcw[6] * pw[0] + Rcw[7] * pw[1] + Rcw[8] * pw[2] + tcw[2];
    if (!(Z >= 1e-3)) return; // :891 (NaN falls out here as it does through allFinite upstream)
    double uu, vv;
    if (!trk_project_cam(cam, X0, X1, Z, uu, vv)) return;
    if (!(fabs(uu) < 2.0e9 && fabs(vv) < 2.0e9)) return; // static_cast<int> of anything larger is undefined upstream
    const int u = (int)uu, v = (int)vv;
    if (u < 0 || u >= width || v < 0 || v >= height) return;
    atomicMin(depth_bits + (int64_t)v * width + u, __float_as_uint((float)Z));
}
__global__ void gm_finish_kernel(int64_t n, unsigned int *__restrict__ bits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && bits[i] == 0x7f800000u) bits[i] = 0u; // untouched pixels: +inf -> 0
}

// ---- per-track fusion: fusion_device.h (host/device-neutral, also run on the CPU by the tests) ----------------------
__global__ void fuse_kernel(int64_t n_tracks, const int64_t *__restrict__ obs_off, const int32_t *__restrict__ obs_img,
                            const float *__restrict__ obs_uv, const float *__restrict__ depth, int width, int height,
                            const double *__restrict__ Rcw, const double *__restrict__ tcw, int32_t n_images, TrkIntr cam,
                            int obser_thr, double cos_min, double reproj_thr, double *__restrict__ pts /*[O][3] scratch*/,
                            double *__restrict__ dirs /*[O][3] scratch*/, uint8_t *__restrict__ flag /*[O] scratch*/,
                            int32_t *__restrict__ idx /*[O][2] scratch*/, uint8_t *__restrict__ status, double *__restrict__ Xout, double *__restrict__ err_out,
                            uint8_t *__restrict__ kept_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tracks) return;
    fuse_track(t, obs_off, obs_img, obs_uv, depth, width, height, Rcw, tcw, n_images, cam, obser_thr, cos_min, reproj_thr, pts, dirs,
               flag, idx, status, Xout, err_out, kept_out);
}

} // namespace

extern "C" int32_t lvba_depth_render(lvba_scans_t sc, const double *scan_poses, const double *scan_times, int32_t n_images,
                                     const double *image_times, const double *Rcw, const double *tcw, const double intr[8],
                                     int32_t width, int32_t height, double half_window_s, double voxel_size, lvba_depth_t *out)
{
    if (out) *out = nullptr;
    if (!sc || !scan_poses || !scan_times || !image_times || !Rcw || !tcw || !intr || !out || n_images < 0 || width < 2 ||
        height < 2 || !(voxel_size > 0) || !(half_window_s >= 0))
        return lvba_fail(LVBA_ERR_ARG, "null or out-of-range argument");
    HIPCHK(hipSetDevice(sc->device));
    const int nf = sc->n_frames;
    const int64_t P = sc->frame_off[nf];
    lvba_depth_s *h = new (std::nothrow) lvba_depth_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    h->device = sc->device; h->n_images = n_images; h->width = width; h->height = height;
    const int64_t npix = (int64_t)width * height;
    {
        void *raw = nullptr;
        hipError_t e = hipMalloc(&raw, (size_t)std::max<int64_t>(1, n_images * npix) * 4);
        if (e != hipSuccess) { delete h; return lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "depth images: %s", hipGetErrorString(e)); }
        h->d_depth = (float *)raw;
    }
    struct Guard { lvba_depth_s *h; ~Guard() { if (h) { (void)hipFree(h->d_depth); delete h; } } } guard{h};
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    if (n_images == 0) { *out = h; guard.h = nullptr; return LVBA_OK; }
    // every pixel starts at +inf
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->d_depth, 0x7f800000, (size_t)(n_images * npix), s));
    if (P > 0) {
        DevArr<double> d_poses(s), world(s); DevArr<uint64_t> key(s); DevArr<uint32_t> idx(s); DevArr<uint64_t> key_s(s);
        DevArr<uint32_t> order(s), head(s), incl(s), vop(s); DevArr<int64_t> voff(s); DevArr<int> d_err(s);
        DevArr<double> d_R(s), d_t(s);
        HIPCHK(d_poses.alloc(12 * (size_t)nf)); HIPCHK(world.alloc(3 * (size_t)P)); HIPCHK(key.alloc((size_t)P));
        HIPCHK(idx.alloc((size_t)P)); HIPCHK(key_s.alloc((size_t)P)); HIPCHK(order.alloc((size_t)P));
        HIPCHK(head.alloc((size_t)P)); HIPCHK(incl.alloc((size_t)P)); HIPCHK(vop.alloc((size_t)P)); HIPCHK(d_err.alloc(1));
        HIPCHK(d_R.alloc(9 * (size_t)n_images)); HIPCHK(d_t.alloc(3 * (size_t)n_images));
        HIPCHK(hipMemcpyAsync(d_poses, scan_poses, d_poses.bytes(12 * (size_t)nf), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_R, Rcw, d_R.bytes(9 * (size_t)n_images), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_t, tcw, d_t.bytes(3 * (size_t)n_images), hipMemcpyHostToDevice, s)); HIPCHK(d_err.zero_async(1));
        gm_world_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, sc->d_pts, sc->d_frame_off, nf, d_poses, voxel_size, world, key, idx,
                                                         d_err);
        HIPCHK(hipGetLastError());
        int err = 0;
        HIPCHK(hipMemcpyAsync(&err, d_err, d_err.bytes(1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (err) return lvba_fail(LVBA_ERR_ARG, "a scan point is non-finite or outside +-2^20 grid voxels");
        TRY(sort_pairs<uint64_t>(s, key, key_s, idx, order, (size_t)P, 63));
        gm_heads_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, key_s, head);
        TRY(scan_incl<uint32_t>(s, head, incl, (size_t)P));
        uint32_t V32 = 0;
        HIPCHK(hipMemcpy(&V32, incl + (P - 1), incl.bytes(1), hipMemcpyDeviceToHost));
        const int64_t V = V32;
        HIPCHK(voff.alloc((size_t)V + 1));
        gm_tables_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, head, incl, order, vop, voff, V);
        HIPCHK(hipGetLastError());
        DevArr<uint32_t> mark(s); DevArr<int64_t> cnt(s), start(s);
        HIPCHK(mark.alloc((size_t)V)); HIPCHK(cnt.alloc((size_t)V + 1)); HIPCHK(start.alloc((size_t)V + 1));
        const TrkIntr cam = trk_intr_of(intr);
        for (int m = 0; m < n_images; ++m) {
            // scans with t_img - half <= t <= t_img + half: std::lower_bound / std::upper_bound on the (sorted) scan times
            const double t0 = image_times[m] - half_window_s, t1 = image_times[m] + half_window_s;
            const int flo = (int)(std::lower_bound(scan_times, scan_times + nf, t0) - scan_times);
            const int fhi = (int)(std::upper_bound(scan_times, scan_times + nf, t1) - scan_times);
            if (fhi <= flo) continue;
            const int64_t p0 = sc->frame_off[flo], np = sc->frame_off[fhi] - p0;
            if (np <= 0) continue;
            HIPCHK(mark.zero_async((size_t)V));
            gm_mark_kernel<<<grid_for(np, 256), 256, 0, s>>>(np, vop + p0, mark);
            gm_count_kernel<<<grid_for(V + 1, 256), 256, 0, s>>>(V, mark, voff, cnt);
            HIPCHK(hipGetLastError());
            TRY(scan_excl<int64_t>(s, cnt, start, (size_t)V + 1));
            int64_t M = 0;
            HIPCHK(hipMemcpy(&M, start + V, start.bytes(1), hipMemcpyDeviceToHost));
            if (M <= 0) continue;
            gm_render_kernel<<<grid_for(M, 256), 256, 0, s>>>(M, V, start, voff, order, world, d_R + 9 * (int64_t)m,
                                                              d_t + 3 * (int64_t)m, cam, width, height,
                                                              reinterpret_cast<unsigned int *>(h->d_depth) + (int64_t)m * npix);
            HIPCHK(hipGetLastError());
        }
    }
    gm_finish_kernel<<<grid_for(n_images * npix, 256), 256, 0, s>>>(n_images * npix, reinterpret_cast<unsigned int *>(h->d_depth));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    *out = h;
    guard.h = nullptr;
    return LVBA_OK;
}

extern "C" int32_t lvba_depth_upload(int32_t device, int32_t n_images, int32_t width, int32_t height, const float *depth,
                                     lvba_depth_t *out)
{
    if (out) *out = nullptr;
    if (!depth || !out || n_images < 1 || width < 2 || height < 2) return lvba_fail(LVBA_ERR_ARG, "null or out-of-range argument");
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_depth_s *h = new (std::nothrow) lvba_depth_s();
    if (!h) return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    h->device = device; h->n_images = n_images; h->width = width; h->height = height;
    const size_t bytes = (size_t)n_images * width * height * 4;
    hipError_t e = hipMalloc((void **)&h->d_depth, bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_depth, depth, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(h->d_depth);
        delete h;
        return lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "depth images: %s", hipGetErrorString(e));
    }
    *out = h;
    return LVBA_OK;
}

extern "C" int32_t lvba_depth_info(lvba_depth_t d, int32_t *n_images, int32_t *width, int32_t *height)
{
    if (!d) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (n_images) *n_images = d->n_images;
    if (width) *width = d->width;
    if (height) *height = d->height;
    return LVBA_OK;
}

extern "C" int32_t lvba_depth_download(lvba_depth_t d, int32_t image, float *depth)
{
    if (!d || !depth || image < 0 || image >= d->n_images) return lvba_fail(LVBA_ERR_ARG, "null handle / image out of range");
    HIPCHK(hipSetDevice(d->device));
    const size_t npix = (size_t)d->width * d->height;
    HIPCHK(hipMemcpy(depth, d->d_depth + (size_t)image * npix, npix * 4, hipMemcpyDeviceToHost));
    return LVBA_OK;
}

extern "C" void lvba_depth_destroy(lvba_depth_t d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipFree(d->d_depth);
    delete d;
}

extern "C" void lvba_fuse_default_opts(lvba_fuse_opts *o)
{
    if (!o) return;
    o->obser_thr = 3;              // config: obser_thr
    o->reserved = 0;
    o->min_view_angle_deg = 8.0;   // config: min_view_angle_deg
    o->reproj_mean_thr_px = 3.0;   // config: reproj_mean_thr_px
}

extern "C" int32_t lvba_fuse_tracks(int32_t device, lvba_depth_t depth, int32_t n_images, const double *Rcw, const double *tcw,
                                    const double intr[8], int64_t n_tracks, const int64_t *obs_off, const int32_t *obs_img,
                                    const float *obs_uv, const lvba_fuse_opts *opts, uint8_t *status, double *X,
                                    double *mean_reproj, uint8_t *kept)
{
    if (n_images < 1 || n_tracks < 0 || !Rcw || !tcw || !intr || !obs_off || !status || !X || !mean_reproj)
        return lvba_fail(LVBA_ERR_ARG, "null argument or n_images < 1");
    if (n_tracks == 0) return LVBA_OK;
    TRY(check_offsets("obs_off", "track", n_tracks, obs_off)); // the kernel walks [obs_off[t], obs_off[t + 1]) of O-element arrays
    const int64_t O = obs_off[n_tracks];
    if (O > 0 && (!obs_img || !obs_uv || !kept)) return lvba_fail(LVBA_ERR_ARG, "bad observation arrays");
    lvba_fuse_opts o;
    lvba_fuse_default_opts(&o);
    if (opts) o = *opts;
    if (o.obser_thr < 1) return lvba_fail(LVBA_ERR_ARG, "obser_thr = %d (>= 1)", o.obser_thr); // fuse_track divides by a count >= obser_thr
    if (!(o.min_view_angle_deg >= 0.0 && o.min_view_angle_deg <= 180.0))
        return lvba_fail(LVBA_ERR_ARG, "min_view_angle_deg = %g (0..180)", o.min_view_angle_deg);
    if (!(o.reproj_mean_thr_px >= 0.0)) return lvba_fail(LVBA_ERR_ARG, "reproj_mean_thr_px = %g (>= 0)", o.reproj_mean_thr_px);
    if (depth) {
        if (depth->n_images != n_images) return lvba_fail(LVBA_ERR_ARG, "depth handle holds %d images, %d cameras given", depth->n_images, n_images);
        device = depth->device;
    }
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    DevArr<int64_t> d_off(s); DevArr<int32_t> d_img(s); DevArr<float> d_uv(s); DevArr<double> d_R(s), d_t(s), d_pts(s), d_dirs(s);
    DevArr<uint8_t> d_flag(s); DevArr<int32_t> d_idx(s); DevArr<uint8_t> d_st(s); DevArr<double> d_X(s), d_err(s);
    DevArr<uint8_t> d_kept(s);
    const size_t O1 = (size_t)std::max<int64_t>(O, 1);
    HIPCHK(d_off.alloc((size_t)n_tracks + 1)); HIPCHK(d_img.alloc(O1)); HIPCHK(d_uv.alloc(2 * O1));
    HIPCHK(d_R.alloc(9 * (size_t)n_images)); HIPCHK(d_t.alloc(3 * (size_t)n_images));
    HIPCHK(d_pts.alloc(3 * O1)); HIPCHK(d_dirs.alloc(3 * O1)); HIPCHK(d_flag.alloc(O1)); HIPCHK(d_idx.alloc(2 * O1));
    HIPCHK(d_st.alloc((size_t)n_tracks)); HIPCHK(d_X.alloc(3 * (size_t)n_tracks)); HIPCHK(d_err.alloc((size_t)n_tracks));
    HIPCHK(d_kept.alloc(O1));
    HIPCHK(hipMemcpyAsync(d_off, obs_off, d_off.bytes((size_t)n_tracks + 1), hipMemcpyHostToDevice, s));
    if (O > 0) {
        HIPCHK(hipMemcpyAsync(d_img, obs_img, d_img.bytes((size_t)O), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_uv, obs_uv, d_uv.bytes(2 * (size_t)O), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(d_R, Rcw, d_R.bytes(9 * (size_t)n_images), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_t, tcw, d_t.bytes(3 * (size_t)n_images), hipMemcpyHostToDevice, s));
    const TrkIntr cam = trk_intr_of(intr);
    const double cos_min = cos(o.min_view_angle_deg * M_PI / 180.0);
    fuse_kernel<<<(unsigned)((n_tracks + 63) / 64), 64, 0, s>>>(
        n_tracks, d_off, d_img, d_uv, depth ? depth->d_depth : nullptr,
        depth ? depth->width : 0, depth ? depth->height : 0, d_R, d_t, n_images, cam, o.obser_thr, cos_min,
        o.reproj_mean_thr_px, d_pts, d_dirs, d_flag, d_idx, d_st, d_X,
        d_err, d_kept);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(status, d_st, d_st.bytes((size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(X, d_X, d_X.bytes(3 * (size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(mean_reproj, d_err, d_err.bytes((size_t)n_tracks), hipMemcpyDeviceToHost, s));
    if (O > 0) HIPCHK(hipMemcpyAsync(kept, d_kept, d_kept.bytes((size_t)O), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return LVBA_OK;
}
