// dynamic.hip -- moving objects in the LiDAR map by range-image visibility (lvba_dynamic_labels) and the compaction of a scan
// set by a per-point mask (lvba_scans_select).  The rule is in include/lvba_hip.h, its scalar arithmetic in dynamic_device.h,
// also compiled for the host by the tests; DESIGN.md §10m.
//
// Device design.  The frames whose images vote are taken in batches of B (all of them when they fit); per batch:
//   dyn_image_kernel    one lane per point of the batch's frames (lane-consecutive 12-byte loads): its frame (frame_of_point), its
//                       cell, and an integer atomicMin of the bits of (float)r into the frame's image, which starts at +inf.
//                       Non-negative floats order like their bits and a minimum does not depend on the order: the same bytes
//                       every call.  (240 x 720 cells are 675 KB a frame: the image lives in global memory, not in LDS.)
//   dyn_dilate_kernel   one lane per cell of the batch: the minimum over its (2 halo + 1)^2 neighbours, lane-consecutive along a
//                       row.
//   dyn_vote_kernel     the hot path.  A workgroup owns a chunk of 256 consecutive points of ONE frame f (the chunk table
//                       chunk_off, searched once per workgroup with segment_of): f, the window bounds and every R_g, t_g of the
//                       loop are workgroup-uniform and come through scalar loads.  A lane owns a point: it forms w = R_f p + t_f
//                       once, keeps w and its two counters in registers, and walks the frames g of the batch inside its window:
//                       nine multiplies, two square roots, two atan2 and one 4-byte gather from M_g per (point, g); neighbours
//                       in a scan land in neighbouring cells.  At the end it adds its counters to the point's totals -- the point
//                       is the lane's alone, the batches follow each other on one stream: no atomics.
//   dyn_label_kernel    one lane per point: the label, and per workgroup the numbers of judged and dynamic points (the integer
//                       DPP tree of wave_ops.h, then four values through LDS); the host adds the workgroups' counts.
// Votes are integer counts: no floating-point sum crosses lanes, and the totals do not depend on the batching.
// lvba_scans_select: flags from the mask, one exclusive scan (rocPRIM), the new frame offsets read off the scan at the old
// ones, one scatter.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "dynamic_device.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int DYN_BLOCK = 256; // the vote kernel's chunk of points

// img [nb][cells] as bits, set to DYN_EMPTY_BITS by the caller; pts / frame_off start at the batch's first frame; n points
__global__ __launch_bounds__(256) void dyn_image_kernel(int64_t n, const float *__restrict__ pts, const int64_t *__restrict__ frame_off,
                                                        int nb, const DynParams o, uint32_t *__restrict__ img)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = frame_of_point(frame_off, nb, i);
    double r;
    const int c = dyn_cell((double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], o, &r);
    if (c >= 0) atomicMin(img + (int64_t)g * ((int64_t)o.n_rows * o.n_cols) + c, __float_as_uint((float)r)); // r >= 0
}

__global__ __launch_bounds__(256) void dyn_dilate_kernel(int64_t n, const DynParams o, const uint32_t *__restrict__ img,
                                                         uint32_t *__restrict__ dil)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t cells = (int64_t)o.n_rows * o.n_cols;
    const int64_t g = i / cells;
    const int c = (int)(i - g * cells);
    dil[i] = dyn_dilate(img + g * cells, o.n_rows, o.n_cols, o.halo, c / o.n_cols, c % o.n_cols);
}

// Workgroup block_first + blockIdx.x of the chunk table: chunk_off [n_frames + 1], frame f has the chunks chunk_off[f] ..
// chunk_off[f + 1] of DYN_BLOCK points.  pts / frame_off / poses start at frame_begin; M holds the frames b0 .. b1 - 1; votes of
// point i (counted from the range's first) are added to n_free[i], n_support[i].
__global__ __launch_bounds__(DYN_BLOCK) void dyn_vote_kernel(const float *__restrict__ pts, const int64_t *__restrict__ frame_off,
                                                             const int64_t *__restrict__ chunk_off, int64_t block_first, int n_frames,
                                                             const double *__restrict__ poses, const float *__restrict__ M, int b0, int b1,
                                                             const DynParams o, int32_t *__restrict__ n_free, int32_t *__restrict__ n_support)
{
    const int64_t blk = block_first + blockIdx.x;
    const int f = segment_of(chunk_off, n_frames, blk); // uniform
    const int64_t base = frame_off[0];
    const int64_t i = frame_off[f] - base + (blk - chunk_off[f]) * DYN_BLOCK + threadIdx.x;
    if (i >= frame_off[f + 1] - base) return;
    int g0, g1;
    dyn_window(f, n_frames, o.window, &g0, &g1);
    const int ga = g0 > b0 ? g0 : b0, gb = g1 < b1 ? g1 : b1;
    double w[3];
    pose_apply(poses + 12 * (int64_t)f, (double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], w);
    int32_t nf = 0, ns = 0;
    dyn_votes(w, f, ga, gb, poses, M, b0, (int64_t)o.n_rows * o.n_cols, o, &nf, &ns);
    n_free[i] += nf;
    n_support[i] += ns;
}

// label [n]; part [gridDim.x][2] = judged, dynamic points of the workgroup
__global__ __launch_bounds__(256) void dyn_label_kernel(int64_t n, const int32_t *__restrict__ n_free, const int32_t *__restrict__ n_support,
                                                        const DynParams o, uint8_t *__restrict__ label, int32_t *__restrict__ part)
{
    __shared__ int32_t red[4][2];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int judged = 0, dynamic = 0;
    if (i < n) {
        const int32_t nf = n_free[i], ns = n_support[i];
        judged = nf + ns > 0 ? 1 : 0;
        dynamic = dyn_label(nf, ns, o);
        label[i] = (uint8_t)dynamic;
    }
    judged = wave_fold_to_lane63<SumStepI32>(judged);
    dynamic = wave_fold_to_lane63<SumStepI32>(dynamic);
    if ((threadIdx.x & 63) == 63) { red[threadIdx.x >> 6][0] = judged; red[threadIdx.x >> 6][1] = dynamic; }
    __syncthreads();
    if (threadIdx.x < 2) part[2 * (int64_t)blockIdx.x + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ---- lvba_scans_select ------------------------------------------------------------------------------------------------------
// flag [n + 1]: keep != 0, and 0 at n, so that the exclusive scan's last entry is the total
__global__ void sel_flag_kernel(int64_t n, const uint8_t *__restrict__ keep, uint32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = i < n && keep[i] ? 1u : 0u;
}
// new_off [n_frames + 1] = excl at the old frame offsets
__global__ void sel_offsets_kernel(int n_frames, const int64_t *__restrict__ frame_off, const uint32_t *__restrict__ excl,
                                   int64_t *__restrict__ new_off)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f <= n_frames) new_off[f] = (int64_t)excl[frame_off[f]];
}
__global__ void sel_scatter_kernel(int64_t n, const float *__restrict__ pts, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                   float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t k = excl[i];
    out[3 * k] = pts[3 * i]; out[3 * k + 1] = pts[3 * i + 1]; out[3 * k + 2] = pts[3 * i + 2];
}

int32_t check_opts(const lvba_dynamic_opts *opts, lvba_dynamic_opts &o, DynParams &p)
{
    lvba_dynamic_default_opts(&o);
    if (opts) o = *opts;
    const double half_pi = 0.5 * PLACE_PI;
    const bool ok = o.n_rows >= 1 && o.n_rows <= DYN_MAX_ROWS && o.n_cols >= 1 && o.n_cols <= DYN_MAX_COLS && o.halo >= 0 &&
                    o.halo <= DYN_MAX_HALO && o.el_min >= -half_pi && o.el_max <= half_pi && o.el_min < o.el_max &&
                    o.min_range >= 0.0 && o.min_range < o.max_range && std::isfinite(o.abs_tol) && o.abs_tol >= 0.0 &&
                    std::isfinite(o.rel_tol) && o.rel_tol >= 0.0 && o.min_free >= 1 && o.free_ratio > 0.0 && o.free_ratio <= 1.0 &&
                    o.batch_frames >= 0;
    if (!ok)
        return lvba_fail(LVBA_ERR_ARG, "options: n_rows %d (1 .. %d), n_cols %d (1 .. %d), halo %d (0 .. %d), el_min %g, el_max %g "
                         "(-pi/2 <= el_min < el_max <= pi/2), min_range %g, max_range %g (0 <= min_range < max_range), abs_tol %g, "
                         "rel_tol %g (finite, >= 0), min_free %d (>= 1), free_ratio %g (in (0, 1]), batch_frames %d (>= 0)",
                         o.n_rows, DYN_MAX_ROWS, o.n_cols, DYN_MAX_COLS, o.halo, DYN_MAX_HALO, o.el_min, o.el_max, o.min_range, o.max_range,
                         o.abs_tol, o.rel_tol, o.min_free, o.free_ratio, o.batch_frames);
    p.n_rows = o.n_rows; p.n_cols = o.n_cols; p.halo = o.halo; p.window = o.window; p.min_free = o.min_free;
    p.el_min = o.el_min; p.el_max = o.el_max; p.min_range = o.min_range; p.max_range = o.max_range;
    p.abs_tol = o.abs_tol; p.rel_tol = o.rel_tol; p.free_ratio = o.free_ratio;
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_dynamic_default_opts(lvba_dynamic_opts *o)
{
    if (!o) return;
    *o = lvba_dynamic_opts{};
    o->n_rows = 240; o->n_cols = 720; o->halo = 1; o->window = 20; o->min_free = 3; o->batch_frames = 0;
    o->el_min = -PLACE_PI / 3.0; o->el_max = PLACE_PI / 3.0;
    o->min_range = 0.5; o->max_range = 80.0; o->abs_tol = 0.2; o->rel_tol = 0.02; o->free_ratio = 0.5;
}

extern "C" int32_t lvba_dynamic_labels(lvba_scans_t sc, const double *scan_poses, int32_t frame_begin, int32_t n_frames,
                                       const lvba_dynamic_opts *opts, lvba_dynamic_summary *summary, uint8_t *label, int32_t *n_free,
                                       int32_t *n_support)
{
    if (!sc || !scan_poses || !summary) return lvba_fail(LVBA_ERR_ARG, "null argument");
    lvba_dynamic_opts o;
    DynParams p;
    TRY(check_opts(opts, o, p));
    if (frame_begin < 0 || n_frames < 1 || (int64_t)frame_begin + n_frames > sc->n_frames)
        return lvba_fail(LVBA_ERR_ARG, "frames [%d, %d + %d) of %d", frame_begin, frame_begin, n_frames, sc->n_frames);
    for (int64_t i = 0; i < 12 * (int64_t)n_frames; ++i)
        if (!std::isfinite(scan_poses[i])) return lvba_fail(LVBA_ERR_ARG, "non-finite scan pose");
    *summary = lvba_dynamic_summary{};
    const int64_t *off = sc->frame_off.data() + frame_begin;
    const int64_t P = off[n_frames] - off[0];
    summary->n_points = P;
    if (P == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(sc->device));
    // the batch: as many frames' images (I and M) as fit beside the per-point arrays, or what the caller asks for
    const int64_t cells = (int64_t)p.n_rows * p.n_cols;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double have = 0.9 * ((double)free_b + (double)DevicePool::get().cached_bytes());
    const double fixed = 9.0 * (double)P + 104.0 * (double)n_frames + 8.0 * (double)(P / DYN_BLOCK + 1) + (double)(1 << 20);
    const double per_frame = 8.0 * (double)cells;
    int B = o.batch_frames > 0 ? std::min(o.batch_frames, n_frames) : n_frames;
    if (o.batch_frames == 0 && fixed + per_frame * B > have) B = (int)std::max(0.0, std::floor((have - fixed) / per_frame));
    if (B < 1 || fixed + per_frame * B > have)
        return lvba_fail(LVBA_ERR_NOMEM, "dynamic labels: %lld points and the images of %d frames need %.0f MB of device memory, %.0f MB are free",
                         (long long)P, std::max(B, 1), (fixed + per_frame * std::max(B, 1)) / 1048576.0, have / 1048576.0);
    // the chunk table of the vote kernel
    std::vector<int64_t> chunk((size_t)n_frames + 1, 0);
    for (int f = 0; f < n_frames; ++f) chunk[(size_t)f + 1] = chunk[(size_t)f] + (off[f + 1] - off[f] + DYN_BLOCK - 1) / DYN_BLOCK;
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<4> ev;
    DevArr<double> d_poses(s); DevArr<int64_t> d_chunk(s); DevArr<uint32_t> d_img(s), d_dil(s);
    DevArr<int32_t> d_nf(s), d_ns(s); DevArr<uint8_t> d_label(s); DevArr<int32_t> d_part(s);
    const unsigned label_grid = grid_for(P, 256);
    HIPCHK(d_poses.alloc(12 * (size_t)n_frames)); HIPCHK(d_chunk.alloc((size_t)n_frames + 1));
    HIPCHK(d_img.alloc((size_t)cells * B)); HIPCHK(d_dil.alloc((size_t)cells * B));
    HIPCHK(d_nf.alloc((size_t)P)); HIPCHK(d_ns.alloc((size_t)P)); HIPCHK(d_label.alloc((size_t)P));
    HIPCHK(d_part.alloc(2 * (size_t)label_grid));
    HIPCHK(hipMemcpyAsync(d_poses, scan_poses, d_poses.bytes(12 * (size_t)n_frames), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_chunk, chunk.data(), d_chunk.bytes((size_t)n_frames + 1), hipMemcpyHostToDevice, s));
    HIPCHK(d_nf.zero_async((size_t)P)); HIPCHK(d_ns.zero_async((size_t)P));
    const float *d_pts = sc->d_pts + 3 * off[0];
    const int64_t *d_off = sc->d_frame_off + frame_begin;
    for (int b0 = 0; b0 < n_frames; b0 += B) {
        const int b1 = std::min(n_frames, b0 + B), nb = b1 - b0;
        const int64_t np = off[b1] - off[b0], nc = cells * nb;
        ev.rec(0, s);
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_img, (int)DYN_EMPTY_BITS, (size_t)nc, s));
        if (np > 0) {
            dyn_image_kernel<<<grid_for(np, 256), 256, 0, s>>>(np, d_pts + 3 * (off[b0] - off[0]), d_off + b0, nb, p, d_img);
            HIPCHK(hipGetLastError());
        }
        ev.rec(1, s);
        dyn_dilate_kernel<<<grid_for(nc, 256), 256, 0, s>>>(nc, p, d_img, d_dil);
        HIPCHK(hipGetLastError());
        ev.rec(2, s);
        // the frames whose window reaches into the batch
        const int fa = p.window <= 0 ? 0 : std::max(0, b0 - p.window), fb = p.window <= 0 ? n_frames : std::min(n_frames, b1 + p.window);
        const int64_t blocks = chunk[(size_t)fb] - chunk[(size_t)fa];
        if (blocks > 0) {
            // d_dil.as<float>(): the range images are written as ordered bit patterns and read as floats
            dyn_vote_kernel<<<(unsigned)blocks, DYN_BLOCK, 0, s>>>(d_pts, d_off, d_chunk, chunk[(size_t)fa], n_frames, d_poses,
                                                                   d_dil.as<float>(), b0, b1, p, d_nf, d_ns);
            HIPCHK(hipGetLastError());
        }
        ev.rec(3, s);
        HIPCHK(hipStreamSynchronize(s));
        summary->ms[0] += ev.ms(0, 1); summary->ms[1] += ev.ms(1, 2); summary->ms[2] += ev.ms(2, 3);
    }
    ev.rec(0, s);
    dyn_label_kernel<<<label_grid, 256, 0, s>>>(P, d_nf, d_ns, p, d_label, d_part);
    HIPCHK(hipGetLastError());
    ev.rec(1, s);
    HIPCHK(hipStreamSynchronize(s));
    summary->ms[2] += ev.ms(0, 1);
    const double t0 = now_ms();
    std::vector<int32_t> part(2 * (size_t)label_grid);
    HIPCHK(d_part.download(part.data(), 2 * (size_t)label_grid));
    for (size_t k = 0; k < (size_t)label_grid; ++k) { summary->n_judged += part[2 * k]; summary->n_dynamic += part[2 * k + 1]; }
    if (label) HIPCHK(d_label.download(label, (size_t)P));
    if (n_free) HIPCHK(d_nf.download(n_free, (size_t)P));
    if (n_support) HIPCHK(d_ns.download(n_support, (size_t)P));
    summary->ms[3] = now_ms() - t0;
    return LVBA_OK;
}

extern "C" int32_t lvba_scans_select(lvba_scans_t sc, const uint8_t *keep, lvba_scans_t *out)
{
    if (out) *out = nullptr;
    if (!sc || !out) return lvba_fail(LVBA_ERR_ARG, "null argument");
    const int nf = sc->n_frames;
    const int64_t P = sc->frame_off[(size_t)nf];
    if (P > 0 && !keep) return lvba_fail(LVBA_ERR_ARG, "null mask");
    if (P >= ((int64_t)1 << 32) - 1) return lvba_fail(LVBA_ERR_ARG, "%lld points (at most 2^32 - 2)", (long long)P);
    HIPCHK(hipSetDevice(sc->device));
    std::vector<int64_t> count((size_t)nf, 0);
    lvba_scans_s *res = nullptr;
    if (P == 0) {
        TRY(scans_build(sc->device, nf, count.data(), nullptr, nullptr, 0, &res));
        *out = res;
        return LVBA_OK;
    }
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    DevArr<uint8_t> d_keep(s); DevArr<uint32_t> d_flag(s), d_excl(s); DevArr<int64_t> d_new(s);
    HIPCHK(d_keep.alloc((size_t)P)); HIPCHK(d_flag.alloc((size_t)P + 1)); HIPCHK(d_excl.alloc((size_t)P + 1));
    HIPCHK(d_new.alloc((size_t)nf + 1)); HIPCHK(d_keep.upload(keep, (size_t)P));
    sel_flag_kernel<<<grid_for(P + 1, 256), 256, 0, s>>>(P, d_keep, d_flag);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, d_flag, d_excl, (size_t)P + 1));
    sel_offsets_kernel<<<grid_for((int64_t)nf + 1, 256), 256, 0, s>>>(nf, sc->d_frame_off, d_excl, d_new);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> new_off((size_t)nf + 1, 0);
    HIPCHK(hipMemcpyAsync(new_off.data(), d_new, d_new.bytes((size_t)nf + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int f = 0; f < nf; ++f) count[(size_t)f] = new_off[(size_t)f + 1] - new_off[(size_t)f];
    TRY(scans_build(sc->device, nf, count.data(), nullptr, nullptr, 0, &res));
    sel_scatter_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, sc->d_pts, d_flag, d_excl, res->d_pts);
    const hipError_t e = hipGetLastError() == hipSuccess ? hipStreamSynchronize(s) : hipErrorUnknown;
    if (e != hipSuccess) {
        lvba_scans_destroy(res);
        return lvba_fail(LVBA_ERR_DEVICE, "scan selection: %s", hipGetErrorString(e));
    }
    *out = res;
    return LVBA_OK;
}
