// sift.hip -- SIFT key points and descriptors of a batch of equally sized images (lvba_sift_*; the rule is in include/lvba_hip.h, its
// scalar pieces in sift_device.h).
//
// Device design (a chunk of C images at a time; grid z = the image of the chunk wherever a kernel works on pixels):
//   sift_base_kernel        a thread per pixel of the base image: grey from the bytes, doubled when first_octave = -1.
//   sift_blur_rows_kernel   a workgroup per 64 x 4 pixels: the rows with a halo of the blur radius in LDS, clamped at the border (the
//                           radius may exceed the image), then the fp32 sum over the taps in ascending order.  The taps of all levels
//                           sit in one small device table that every image of the call shares.
//   sift_blur_cols_kernel   the same down the columns, a workgroup per 64 x 16 pixels.
//   sift_decimate_kernel    level S at every second pixel: the first level of the next octave.
//   sift_detect_kernel      a thread per pixel walks up the levels with three 3 x 3 DoG windows in registers: it writes the DoG value
//                           of every level (the refinement reads them) and the 26-neighbour flag of levels 1 .. S.
//   (exclusive scan of the flags) + sift_gather_kernel: the candidates in (image, level, y, x) order -- the canonical order.
//   sift_refine_kernel      a lane per candidate: the fp64 fit of sift_device.h.
//   sift_orient_kernel      a wavefront per candidate.  Round by round every lane evaluates one sample of the window (its bin and
//                           weighted magnitude go to LDS); then lane b < 36 walks the 64 samples in order and adds those of bin b.
//                           Every bin is thus summed in the window's row-major order by ONE lane: no atomics, no reduction tree, and
//                           the order of the sum is the rule's.  Lane 0 smooths and picks the peaks.
//   (exclusive scan of the orientation counts: a feature's place in the output)
//   sift_describe_kernel    a wavefront per candidate, once per orientation: the same scheme with 128 bins, two per lane.  The lane
//                           that has a sample shares its magnitude among the four cells once; the lane that owns a bin takes its
//                           cell's share times the direction's weight.  Lane 0 normalises and quantises, every lane stores two bytes.
// The pyramid of a chunk stays on the device and is reused octave by octave.  What depends on the image alone decides every
// byte: a pair of calls, a batch, a batch reversed and any chunk size give the same bytes per image.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "sift_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int TAPS_STRIDE = 2 * SIFT_MAX_RADIUS + 1;
constexpr int SIFT_MAX_SIDE = 16384;
constexpr int SIFT_MAX_CHUNK = 64;

struct SiftCand {
    int32_t img, x, y, l;      // image of the chunk; the sample the fit ended on
    int32_t ok, n_ori;
    double ox, oy, ol, sig;    // the offset; the scale inside the octave
    float theta[SIFT_MAX_ORI];
};

__device__ __forceinline__ float grey_at(const uint8_t *p, int w, int ch, int x, int y)
{
    const uint8_t *q = p + ((int64_t)y * w + x) * ch;
    if (ch == 1) return (float)q[0] / 255.0f;
    return ((0.299f * (float)q[2] + 0.587f * (float)q[1]) + 0.114f * (float)q[0]) / 255.0f;
}

// out [C][H][W], (W, H) = (2 w, 2 h) when doubled
__global__ __launch_bounds__(256) void sift_base_kernel(const uint8_t *__restrict__ img, int w, int h, int ch, int doubled,
                                                        float *__restrict__ out)
{
    const int W = doubled ? 2 * w : w, H = doubled ? 2 * h : h;
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X >= W || Y >= H) return;
    const uint8_t *p = img + (int64_t)blockIdx.z * w * h * ch;
    float v;
    if (!doubled) {
        v = grey_at(p, w, ch, X, Y);
    } else {
        const int x0 = X >> 1, x1 = min(x0 + 1, w - 1), y0 = Y >> 1, y1 = min(y0 + 1, h - 1);
        const float a = (X & 1) ? 0.5f * (grey_at(p, w, ch, x0, y0) + grey_at(p, w, ch, x1, y0)) : grey_at(p, w, ch, x0, y0);
        if (Y & 1) {
            const float b = (X & 1) ? 0.5f * (grey_at(p, w, ch, x0, y1) + grey_at(p, w, ch, x1, y1)) : grey_at(p, w, ch, x0, y1);
            v = 0.5f * (a + b);
        } else {
            v = a;
        }
    }
    out[((int64_t)blockIdx.z * H + Y) * W + X] = v;
}

// taps [2 r + 1]; src / dst: image z at z * stride
__global__ __launch_bounds__(256) void sift_blur_rows_kernel(const float *__restrict__ src, int64_t src_stride, float *__restrict__ dst,
                                                             int64_t dst_stride, int w, int h, const float *__restrict__ taps, int r)
{
    __shared__ float tile[4][SIFT_TILE + 2 * SIFT_MAX_RADIUS];
    const int tx = threadIdx.x, ty = threadIdx.y, x0 = blockIdx.x * SIFT_TILE, y = blockIdx.y * 4 + ty;
    const float *s = src + (int64_t)blockIdx.z * src_stride + (int64_t)min(y, h - 1) * w;
    for (int k = tx; k < SIFT_TILE + 2 * r; k += SIFT_TILE) tile[ty][k] = s[min(max(x0 + k - r, 0), w - 1)];
    __syncthreads();
    const int x = x0 + tx;
    if (x >= w || y >= h) return;
    float acc = taps[0] * tile[ty][tx];
    for (int k = 1; k <= 2 * r; ++k) acc = acc + taps[k] * tile[ty][tx + k];
    dst[(int64_t)blockIdx.z * dst_stride + (int64_t)y * w + x] = acc;
}

__global__ __launch_bounds__(256) void sift_blur_cols_kernel(const float *__restrict__ src, int64_t src_stride, float *__restrict__ dst,
                                                             int64_t dst_stride, int w, int h, const float *__restrict__ taps, int r)
{
    __shared__ float tile[SIFT_TILE_ROWS + 2 * SIFT_MAX_RADIUS][SIFT_TILE];
    const int tx = threadIdx.x, ty = threadIdx.y, x = blockIdx.x * SIFT_TILE + tx, y0 = blockIdx.y * SIFT_TILE_ROWS;
    const float *s = src + (int64_t)blockIdx.z * src_stride + min(x, w - 1);
    for (int k = ty; k < SIFT_TILE_ROWS + 2 * r; k += 4) tile[k][tx] = s[(int64_t)min(max(y0 + k - r, 0), h - 1) * w];
    __syncthreads();
    if (x >= w) return;
    for (int m = ty; m < SIFT_TILE_ROWS; m += 4) {
        const int y = y0 + m;
        if (y >= h) break;
        float acc = taps[0] * tile[m][tx];
        for (int k = 1; k <= 2 * r; ++k) acc = acc + taps[k] * tile[m + k][tx];
        dst[(int64_t)blockIdx.z * dst_stride + (int64_t)y * w + x] = acc;
    }
}

// dst [C][h2][w2] (image z at z * dst_stride) = src (w wide) at every second pixel
__global__ __launch_bounds__(256) void sift_decimate_kernel(const float *__restrict__ src, int64_t src_stride, int w, float *__restrict__ dst,
                                                            int64_t dst_stride, int w2, int h2)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w2 || y >= h2) return;
    dst[(int64_t)blockIdx.z * dst_stride + (int64_t)y * w2 + x] = src[(int64_t)blockIdx.z * src_stride + (int64_t)(2 * y) * w + 2 * x];
}

__global__ __launch_bounds__(256) void sift_copy_kernel(const float *__restrict__ src, int64_t src_stride, float *__restrict__ dst,
                                                        int64_t dst_stride, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(int64_t)blockIdx.z * dst_stride + i] = src[(int64_t)blockIdx.z * src_stride + i];
}

// gauss [C][S + 3][h][w] -> dog [C][S + 2][h][w], flag [C][S][h][w] (DoG levels 1 .. S)
__global__ __launch_bounds__(256) void sift_detect_kernel(const float *__restrict__ gauss, float *__restrict__ dog, uint32_t *__restrict__ flag,
                                                          int w, int h, int S, double thr)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int64_t npx = (int64_t)w * h, pix = (int64_t)y * w + x;
    const float *G = gauss + (int64_t)blockIdx.z * (S + 3) * npx;
    float *D = dog + (int64_t)blockIdx.z * (S + 2) * npx;
    uint32_t *F = flag + (int64_t)blockIdx.z * S * npx;
    const bool interior = x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2;
    int64_t at[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) at[k] = (int64_t)min(max(y + k / 3 - 1, 0), h - 1) * w + min(max(x + k % 3 - 1, 0), w - 1);
    float ga[9], d0[9], d1[9], d2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { ga[k] = G[at[k]]; d0[k] = d1[k] = 0.f; }
    for (int l = 0; l < S + 2; ++l) {
        const float *Gn = G + (int64_t)(l + 1) * npx;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float gb = Gn[at[k]];
            d2[k] = gb - ga[k];
            ga[k] = gb;
        }
        D[(int64_t)l * npx + pix] = d2[4];
        if (l >= 2) { // d1 is DoG level l - 1 in 1 .. S
            const float v = d1[4];
            bool hit = interior && (double)fabsf(v) > thr;
            if (hit) {
                bool gt = true, lt = true;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    gt = gt && v > d0[k] && v > d2[k];
                    lt = lt && v < d0[k] && v < d2[k];
                    if (k != 4) { gt = gt && v > d1[k]; lt = lt && v < d1[k]; }
                }
                hit = gt || lt;
            }
            F[(int64_t)(l - 2) * npx + pix] = hit ? 1u : 0u;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) { d0[k] = d1[k]; d1[k] = d2[k]; }
    }
}

__global__ __launch_bounds__(256) void sift_gather_kernel(int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                          int64_t *__restrict__ cand)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) cand[excl[i]] = i;
}

__global__ __launch_bounds__(256) void sift_refine_kernel(int64_t n, const int64_t *__restrict__ cand, const float *__restrict__ dog, int w, int h,
                                                          int S, double sigma0, double dog_threshold, double edge, SiftCand *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int64_t npx = (int64_t)w * h, idx = cand[c];
    const int img = (int)(idx / (S * npx));
    const int64_t rem = idx - (int64_t)img * S * npx;
    int l = (int)(rem / npx) + 1;
    const int64_t pix = rem - (int64_t)(l - 1) * npx;
    int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
    SiftCand k{};
    k.img = img;
    double ox = 0.0, oy = 0.0, ol = 0.0;
    k.ok = sift_refine(dog + (int64_t)img * (S + 2) * npx, w, h, S, dog_threshold, edge, x, y, l, ox, oy, ol) ? 1 : 0;
    k.x = x; k.y = y; k.l = l; k.ox = ox; k.oy = oy; k.ol = ol;
    k.sig = k.ok ? sift_octave_sigma(sigma0, S, l, ol) : 0.0;
    out[c] = k;
}

// one wavefront per candidate
__global__ __launch_bounds__(64) void sift_orient_kernel(int64_t n, SiftCand *__restrict__ cands, const float *__restrict__ gauss, int w, int h,
                                                         int S, double window, int max_ori, uint32_t *__restrict__ n_ori)
{
    __shared__ int s_bin[64];
    __shared__ double s_val[64];
    __shared__ double hist[SIFT_ORI_BINS], tmp[SIFT_ORI_BINS];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    SiftCand &k = cands[c];
    if (!k.ok) { // the whole wavefront
        if (lane == 0) { k.n_ori = 0; n_ori[c] = 0; }
        return;
    }
    const int64_t npx = (int64_t)w * h;
    const float *G = gauss + ((int64_t)k.img * (S + 3) + k.l) * npx;
    const int x = k.x, y = k.y;
    const double ox = k.ox, oy = k.oy, sig = k.sig;
    const int R = sift_ori_radius(window, sig), side = 2 * R + 1, total = side * side;
    double acc = 0.0;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        int bin = -1;
        double val = 0.0;
        if (t < total && !sift_ori_sample(G, w, h, x, y, t % side - R, t / side - R, R, ox, oy, sig, bin, val)) bin = -1;
        s_bin[lane] = bin; s_val[lane] = val;
        __syncthreads();
        if (lane < SIFT_ORI_BINS)
            for (int j = 0; j < 64; ++j)
                if (s_bin[j] == lane) acc = acc + s_val[j];
        __syncthreads();
    }
    if (lane < SIFT_ORI_BINS) hist[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double theta[SIFT_MAX_ORI];
        const int m = sift_ori_peaks(hist, tmp, max_ori, theta);
        for (int q = 0; q < SIFT_MAX_ORI; ++q) k.theta[q] = q < m ? (float)theta[q] : 0.f;
        k.n_ori = m;
        n_ori[c] = (uint32_t)m;
    }
}

// one wavefront per candidate; its orientation q is feature excl[c] + q.  scale = 2^o; kp [n_feat][4], desc [n_feat][128], img [n_feat]
__global__ __launch_bounds__(64) void sift_describe_kernel(int64_t n, const SiftCand *__restrict__ cands, const uint32_t *__restrict__ excl,
                                                           const float *__restrict__ gauss, int w, int h, int S, double scale,
                                                           float *__restrict__ kp, uint8_t *__restrict__ desc, int32_t *__restrict__ img)
{
    __shared__ SiftDescSample smp[64];
    __shared__ int s_ok[64];
    __shared__ double acc_s[SIFT_DESC];
    __shared__ uint8_t bytes[SIFT_DESC];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const SiftCand &k = cands[c];
    if (!k.ok || k.n_ori == 0) return; // the whole wavefront
    const int64_t npx = (int64_t)w * h;
    const float *G = gauss + ((int64_t)k.img * (S + 3) + k.l) * npx;
    const int x = k.x, y = k.y;
    const double ox = k.ox, oy = k.oy, sig = k.sig;
    const int R = sift_desc_radius(sig), side = 2 * R + 1, total = side * side;
    const int br = lane >> 4, bc = (lane >> 2) & 3, bo = 2 * (lane & 3); // the lane's bins: (br, bc, bo) and (br, bc, bo + 1) = 2 lane, + 1
    for (int q = 0; q < k.n_ori; ++q) {
        const double theta = (double)k.theta[q], ct = cos(theta), st = sin(theta);
        double a0 = 0.0, a1 = 0.0;
        for (int t0 = 0; t0 < total; t0 += 64) {
            const int t = t0 + lane;
            SiftDescSample s;
            const bool ok = t < total && sift_desc_sample(G, w, h, x, y, t % side - R, t / side - R, ox, oy, sig, theta, ct, st, s);
            s_ok[lane] = ok ? 1 : 0;
            if (ok) smp[lane] = s;
            __syncthreads();
            for (int j = 0; j < 64; ++j) {
                if (!s_ok[j]) continue; // (the same j in every lane)
                const int dr = br - smp[j].r0, dc = bc - smp[j].c0;
                if ((unsigned)dr > 1u || (unsigned)dc > 1u) continue;
                // sift_desc_share for the lane's two directions, the cell's share read once
                const int o0 = smp[j].o0, o1 = (o0 + 1) & 7;
                if (o0 != bo && o0 != bo + 1 && o1 != bo && o1 != bo + 1) continue;
                const double p = smp[j].p[2 * dr + dc], fo = smp[j].fo;
                if (o0 == bo) a0 = a0 + p * (1.0 - fo); else if (o1 == bo) a0 = a0 + p * fo;
                if (o0 == bo + 1) a1 = a1 + p * (1.0 - fo); else if (o1 == bo + 1) a1 = a1 + p * fo;
            }
            __syncthreads();
        }
        acc_s[2 * lane] = a0; acc_s[2 * lane + 1] = a1;
        __syncthreads();
        if (lane == 0) sift_desc_bytes(acc_s, bytes);
        __syncthreads();
        const int64_t f = (int64_t)excl[c] + q;
        desc[f * SIFT_DESC + 2 * lane] = bytes[2 * lane];
        desc[f * SIFT_DESC + 2 * lane + 1] = bytes[2 * lane + 1];
        if (lane == 0) {
            kp[4 * f] = (float)(((double)x + ox) * scale);
            kp[4 * f + 1] = (float)(((double)y + oy) * scale);
            kp[4 * f + 2] = (float)(sig * scale);
            kp[4 * f + 3] = k.theta[q];
            img[f] = k.img;
        }
        __syncthreads();
    }
}

// ---- host side

double level_sigma(const lvba_sift_opts &o, int level)
{
    if (level == 0) {
        const double assumed = o.first_octave < 0 ? 1.0 : 0.5;
        return std::sqrt(o.sigma0 * o.sigma0 - assumed * assumed);
    }
    const double S = (double)o.n_intervals;
    return o.sigma0 * std::pow(2.0, (double)(level - 1) / S) * std::sqrt(std::pow(2.0, 2.0 / S) - 1.0);
}

int taps_for(const lvba_sift_opts &o, int level, float *taps)
{
    const double sigma = level_sigma(o, level);
    const int r = (int)std::ceil(4.0 * sigma);
    if (r > SIFT_MAX_RADIUS || r < 1) return -1;
    double g[TAPS_STRIDE], sum = 0.0;
    for (int k = -r; k <= r; ++k) {
        g[k + r] = std::exp(-((double)k * (double)k) / (2.0 * sigma * sigma));
        sum += g[k + r];
    }
    if (taps)
        for (int k = 0; k <= 2 * r; ++k) taps[k] = (float)(g[k] / sum);
    return r;
}

int32_t check_opts(const lvba_sift_opts *opts, lvba_sift_opts &o)
{
    lvba_sift_default_opts(&o);
    if (opts) o = *opts;
    bool ok = (o.first_octave == -1 || o.first_octave == 0) && o.n_intervals >= 2 && o.n_intervals <= SIFT_MAX_INTERVALS &&
              std::isfinite(o.sigma0) && o.sigma0 >= 1.1 && o.sigma0 <= 4.0 && std::isfinite(o.dog_threshold) && o.dog_threshold > 0.0 &&
              o.dog_threshold <= 1.0 && std::isfinite(o.edge_threshold) && o.edge_threshold >= 1.0 && o.edge_threshold <= 1000.0 &&
              std::isfinite(o.orientation_window) && o.orientation_window >= 0.5 && o.orientation_window <= 6.0 && o.max_orientations >= 1 &&
              o.max_orientations <= SIFT_MAX_ORI && o.max_features >= 1 && o.chunk_images >= 0 && o.reserved == 0;
    if (ok)
        for (int l = 0; l <= o.n_intervals + 2; ++l) ok = ok && taps_for(o, l, nullptr) > 0;
    if (!ok)
        return lvba_fail(LVBA_ERR_ARG, "options: first_octave %d (-1 or 0), n_intervals %d (2 .. %d), sigma0 %g (in [1.1, 4], every blur "
                         "radius ceil(4 sigma) <= %d), dog_threshold %g (in (0, 1]), edge_threshold %g (in [1, 1000]), orientation_window %g "
                         "(in [0.5, 6]), max_orientations %d (1 .. %d), max_features %d (>= 1), chunk_images %d (>= 0), reserved %d (0)",
                         o.first_octave, o.n_intervals, SIFT_MAX_INTERVALS, o.sigma0, SIFT_MAX_RADIUS, o.dog_threshold, o.edge_threshold,
                         o.orientation_window, o.max_orientations, SIFT_MAX_ORI, o.max_features, o.chunk_images, o.reserved);
    return LVBA_OK;
}

int32_t check_image(int32_t width, int32_t height, int32_t channels)
{
    if (width < 8 || height < 8 || width > SIFT_MAX_SIDE || height > SIFT_MAX_SIDE || (channels != 1 && channels != 3))
        return lvba_fail(LVBA_ERR_ARG, "images of %d x %d pixels (8 .. %d each way) with %d channels (1 or 3)", width, height, SIFT_MAX_SIDE,
                         channels);
    return LVBA_OK;
}

struct Feature { float kp[4]; uint8_t desc[SIFT_DESC]; };

// host-clock times of the last lvba_sift_extract of this thread, taken where the stream is drained anyway (and once after every
// octave's levels): pyramid (upload, base image, blurs), detection (DoG, flags, scan, refinement), orientation, descriptor
// (with the download), assembly on the host, the whole call
thread_local double g_sift_ms[6] = {0, 0, 0, 0, 0, 0};

// The pyramid of one chunk of images and the passes over it.
struct SiftChunk {
    hipStream_t s;
    lvba_sift_opts o;
    int w_in, h_in, ch, C = 0, S;
    std::vector<int> ow, oh;         // octave sizes
    int oct = -1;                    // the octave the buffers hold
    DevArr<uint8_t> d_img; DevArr<float> d_gauss, d_dog, d_tmp; DevArr<uint32_t> d_flag, d_excl; DevArr<float> d_taps;
    DevArr<int64_t> d_cand_idx; DevArr<SiftCand> d_cand;
    int radius[SIFT_MAX_INTERVALS + 3];
    int64_t n_cand = 0;

    SiftChunk(hipStream_t st, const lvba_sift_opts &opts, int w, int h, int channels)
        : s(st), o(opts), w_in(w), h_in(h), ch(channels), S(opts.n_intervals), d_img(st), d_gauss(st), d_dog(st), d_tmp(st), d_flag(st),
          d_excl(st), d_taps(st), d_cand_idx(st), d_cand(st)
    {
        int cw = o.first_octave < 0 ? 2 * w : w, chh = o.first_octave < 0 ? 2 * h : h;
        do {
            ow.push_back(cw); oh.push_back(chh);
            cw /= 2; chh /= 2;
        } while (std::min(cw, chh) >= 8);
    }
    int n_octaves() const { return (int)ow.size(); }
    int64_t npx0() const { return (int64_t)ow[0] * oh[0]; }
    // device bytes that one image of a chunk needs
    size_t bytes_per_image() const
    {
        return (size_t)w_in * h_in * ch + 4 * (size_t)npx0() * ((S + 3) + (S + 2) + 1 + 2 * S) + 64;
    }
    int32_t alloc(int chunk)
    {
        C = chunk;
        const size_t n0 = (size_t)npx0() * C;
        HIPCHK(d_img.alloc((size_t)w_in * h_in * ch * C));
        HIPCHK(d_gauss.alloc(n0 * (S + 3))); HIPCHK(d_dog.alloc(n0 * (S + 2))); HIPCHK(d_tmp.alloc(n0));
        HIPCHK(d_flag.alloc(n0 * S + 1)); HIPCHK(d_excl.alloc(n0 * S + 1));
        std::vector<float> taps((size_t)TAPS_STRIDE * (S + 3), 0.f);
        for (int l = 0; l <= S + 2; ++l) radius[l] = taps_for(o, l, &taps[(size_t)TAPS_STRIDE * l]);
        HIPCHK(d_taps.alloc_upload(taps));
        return LVBA_OK;
    }
    dim3 grid(int w, int h, int rows, int n) const { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + rows - 1) / rows), (unsigned)n); }
    int32_t blur(const float *src, int64_t src_stride, float *dst, int64_t dst_stride, int w, int h, int level, int n)
    {
        const float *taps = d_taps + (size_t)TAPS_STRIDE * level;
        sift_blur_rows_kernel<<<grid(w, h, 4, n), dim3(64, 4), 0, s>>>(src, src_stride, d_tmp, (int64_t)w * h, w, h, taps,
                                                                      radius[level]);
        HIPCHK(hipGetLastError());
        sift_blur_cols_kernel<<<grid(w, h, SIFT_TILE_ROWS, n), dim3(64, 4), 0, s>>>(d_tmp, (int64_t)w * h, dst, dst_stride, w, h,
                                                                                   taps, radius[level]);
        HIPCHK(hipGetLastError());
        return LVBA_OK;
    }
    // images: n <= C images of the caller's; afterwards the buffers hold octave 0
    int32_t begin(const uint8_t *images, int n)
    {
        C = n;
        HIPCHK(d_img.upload(images, (size_t)w_in * h_in * ch * n));
        const int w = ow[0], h = oh[0];
        const int64_t npx = (int64_t)w * h;
        sift_base_kernel<<<grid(w, h, 4, n), dim3(64, 4), 0, s>>>(d_img, w_in, h_in, ch, o.first_octave < 0 ? 1 : 0,
                                                                 d_dog);
        HIPCHK(hipGetLastError());
        TRY(blur(d_dog, npx, d_gauss, (S + 3) * npx, w, h, 0, n));
        oct = 0;
        return levels();
    }
    // levels 1 .. S + 2 of the current octave from its level 0
    int32_t levels()
    {
        const int w = ow[oct], h = oh[oct];
        const int64_t npx = (int64_t)w * h, stride = (S + 3) * npx;
        for (int l = 1; l <= S + 2; ++l)
            TRY(blur(d_gauss + (l - 1) * npx, stride, d_gauss + l * npx, stride, w, h, l, C));
        return LVBA_OK;
    }
    int32_t next_octave()
    {
        const int w = ow[oct], h = oh[oct], w2 = ow[oct + 1], h2 = oh[oct + 1];
        const int64_t npx = (int64_t)w * h, npx2 = (int64_t)w2 * h2;
        sift_decimate_kernel<<<grid(w2, h2, 4, C), dim3(64, 4), 0, s>>>(d_gauss + S * npx, (S + 3) * npx, w, d_tmp, npx2,
                                                                       w2, h2);
        HIPCHK(hipGetLastError());
        sift_copy_kernel<<<dim3(grid_for(npx2, 256), 1, (unsigned)C), 256, 0, s>>>(d_tmp, npx2, d_gauss, (S + 3) * npx2,
                                                                                  npx2);
        HIPCHK(hipGetLastError());
        ++oct;
        return levels();
    }
    // DoG levels and candidates of the current octave, refined: d_cand [n_cand]
    int32_t detect()
    {
        const int w = ow[oct], h = oh[oct];
        const int64_t n = (int64_t)w * h * S * C;
        sift_detect_kernel<<<grid(w, h, 4, C), dim3(64, 4), 0, s>>>(d_gauss, d_dog, d_flag, w, h, S,
                                                                   (0.5 * o.dog_threshold) / (double)S);
        HIPCHK(hipGetLastError());
        TRY(count_flags(s, d_flag, d_excl, (size_t)n, &n_cand));
        if (n_cand == 0) return LVBA_OK;
        d_cand_idx.reset(); d_cand.reset(); // (each drains the stream before its block goes back)
        HIPCHK(d_cand_idx.alloc((size_t)n_cand)); HIPCHK(d_cand.alloc((size_t)n_cand));
        sift_gather_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, d_flag, d_excl, d_cand_idx);
        HIPCHK(hipGetLastError());
        sift_refine_kernel<<<grid_for(n_cand, 256), 256, 0, s>>>(n_cand, d_cand_idx, d_dog, w, h, S, o.sigma0,
                                                               o.dog_threshold, o.edge_threshold, d_cand);
        HIPCHK(hipGetLastError());
        return LVBA_OK;
    }
    double scale() const { return std::ldexp(1.0, o.first_octave + oct); }
    // orientations and descriptors of the refined candidates; the features are appended to out[image of the chunk]
    int32_t describe(std::vector<std::vector<Feature>> &out)
    {
        if (n_cand == 0) return LVBA_OK;
        const int w = ow[oct], h = oh[oct];
        // d_flag / d_excl are free again: the orientation counts and their scan
        uint32_t *d_n = d_flag, *d_first = d_excl;
        const double t0 = now_ms();
        sift_orient_kernel<<<(unsigned)n_cand, 64, 0, s>>>(n_cand, d_cand, d_gauss, w, h, S, o.orientation_window,
                                                         o.max_orientations, d_n);
        HIPCHK(hipGetLastError());
        int64_t n_feat = 0;
        TRY(count_flags(s, d_n, d_first, (size_t)n_cand, &n_feat));
        const double t1 = now_ms();
        g_sift_ms[2] += t1 - t0;
        if (n_feat == 0) return LVBA_OK;
        DevArr<float> d_kp(s); DevArr<uint8_t> d_desc(s); DevArr<int32_t> d_im(s);
        HIPCHK(d_kp.alloc(4 * (size_t)n_feat)); HIPCHK(d_desc.alloc((size_t)SIFT_DESC * n_feat)); HIPCHK(d_im.alloc((size_t)n_feat));
        sift_describe_kernel<<<(unsigned)n_cand, 64, 0, s>>>(n_cand, d_cand, d_first, d_gauss, w, h, S, scale(),
                                                           d_kp, d_desc, d_im);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        std::vector<float> kp(4 * (size_t)n_feat);
        std::vector<uint8_t> desc((size_t)SIFT_DESC * n_feat);
        std::vector<int32_t> im((size_t)n_feat);
        HIPCHK(d_kp.download(kp.data(), 4 * (size_t)n_feat)); HIPCHK(d_desc.download(desc.data(), desc.size()));
        HIPCHK(d_im.download(im.data(), (size_t)n_feat));
        for (int64_t f = 0; f < n_feat; ++f) {
            Feature ft;
            std::copy_n(&kp[4 * (size_t)f], 4, ft.kp);
            std::copy_n(&desc[(size_t)SIFT_DESC * f], SIFT_DESC, ft.desc);
            out[(size_t)im[(size_t)f]].push_back(ft);
        }
        g_sift_ms[3] += now_ms() - t1;
        return LVBA_OK;
    }
};

// the chunk size: the caller's, or what half of the free device memory holds
int32_t pick_chunk(const SiftChunk &c, int32_t n_images, int *chunk)
{
    int n = c.o.chunk_images;
    if (n == 0) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        n = (int)std::min<size_t>(SIFT_MAX_CHUNK, (free_b / 2) / c.bytes_per_image());
    }
    *chunk = std::max(1, std::min(n, n_images));
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_sift_default_opts(lvba_sift_opts *o)
{
    if (!o) return;
    *o = lvba_sift_opts{};
    o->first_octave = -1; o->n_intervals = 3; o->sigma0 = 1.6; o->dog_threshold = 0.01; o->edge_threshold = 12.0;
    o->orientation_window = 3.0; o->max_orientations = 2; o->max_features = 8192; o->chunk_images = 0;
}

extern "C" int32_t lvba_sift_tile_width(void) { return SIFT_TILE; }

extern "C" int32_t lvba_sift_blur_taps(const lvba_sift_opts *opts, int32_t level, float *taps, int32_t *radius)
{
    if (!taps || !radius) return lvba_fail(LVBA_ERR_ARG, "null output");
    lvba_sift_opts o;
    TRY(check_opts(opts, o));
    if (level < 0 || level > o.n_intervals + 2) return lvba_fail(LVBA_ERR_ARG, "level %d (0 .. %d)", level, o.n_intervals + 2);
    *radius = taps_for(o, level, taps);
    return LVBA_OK;
}

extern "C" int32_t lvba_sift_extract(int32_t device, int32_t n_images, int32_t width, int32_t height, int32_t channels, const uint8_t *images,
                                     const lvba_sift_opts *opts, int64_t capacity, int64_t *feat_off, float *keypoints, uint8_t *descriptors,
                                     int64_t *count)
{
    if (n_images < 0 || capacity < 0 || !feat_off || (n_images > 0 && (!images || !count)) || (capacity > 0 && (!keypoints || !descriptors)))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_images < 0 or capacity < 0");
    TRY(check_image(width, height, channels));
    lvba_sift_opts o;
    TRY(check_opts(opts, o));
    if (n_images == 0) { feat_off[0] = 0; return LVBA_OK; }
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    std::vector<std::vector<Feature>> feats((size_t)n_images);
    const double t_call = now_ms();
    std::fill(g_sift_ms, g_sift_ms + 6, 0.0);
    {
        SiftChunk ck(sg.s, o, width, height, channels);
        int chunk = 1;
        TRY(pick_chunk(ck, n_images, &chunk));
        TRY(ck.alloc(chunk));
        const size_t img_bytes = (size_t)width * height * channels;
        for (int i0 = 0; i0 < n_images; i0 += chunk) {
            const int n = std::min(chunk, n_images - i0);
            std::vector<std::vector<Feature>> part((size_t)n);
            double t = now_ms();
            TRY(ck.begin(images + img_bytes * i0, n));
            for (int k = 0;; ++k) {
                HIPCHK(hipStreamSynchronize(sg.s));
                g_sift_ms[0] += now_ms() - t;
                t = now_ms();
                TRY(ck.detect());
                HIPCHK(hipStreamSynchronize(sg.s));
                g_sift_ms[1] += now_ms() - t;
                TRY(ck.describe(part));
                if (k + 1 == ck.n_octaves()) break;
                t = now_ms();
                TRY(ck.next_octave());
            }
            for (int i = 0; i < n; ++i) feats[(size_t)(i0 + i)] = std::move(part[(size_t)i]);
        }
    }
    const double t_host = now_ms();
    int64_t base = 0;
    feat_off[0] = 0;
    for (int i = 0; i < n_images; ++i) {
        const std::vector<Feature> &f = feats[(size_t)i];
        count[i] = (int64_t)f.size();
        std::vector<int64_t> keep(f.size());
        std::iota(keep.begin(), keep.end(), 0);
        if ((int64_t)f.size() > o.max_features) { // the largest sigma, a tie to the earlier; back into the canonical order
            std::stable_sort(keep.begin(), keep.end(), [&](int64_t a, int64_t b) { return f[(size_t)a].kp[2] > f[(size_t)b].kp[2]; });
            keep.resize((size_t)o.max_features);
            std::sort(keep.begin(), keep.end());
        }
        for (int64_t j : keep) {
            if (base < capacity) {
                std::copy_n(f[(size_t)j].kp, 4, keypoints + 4 * base);
                std::copy_n(f[(size_t)j].desc, SIFT_DESC, descriptors + (int64_t)SIFT_DESC * base);
            }
            ++base;
        }
        feat_off[i + 1] = base;
    }
    g_sift_ms[4] = now_ms() - t_host;
    g_sift_ms[5] = now_ms() - t_call;
    return LVBA_OK;
}

extern "C" int32_t lvba_sift_profile(double *ms)
{
    if (!ms) return lvba_fail(LVBA_ERR_ARG, "null output");
    std::copy_n(g_sift_ms, 6, ms);
    return LVBA_OK;
}

extern "C" int32_t lvba_sift_pyramid(int32_t device, int32_t width, int32_t height, int32_t channels, const uint8_t *image,
                                     const lvba_sift_opts *opts, int32_t octave, float *gauss, float *dog)
{
    if (!image || !gauss || !dog) return lvba_fail(LVBA_ERR_ARG, "null argument");
    TRY(check_image(width, height, channels));
    lvba_sift_opts o;
    TRY(check_opts(opts, o));
    const int k = octave - o.first_octave;
    {
        SiftChunk probe(nullptr, o, width, height, channels);
        if (k < 0 || k >= probe.n_octaves())
            return lvba_fail(LVBA_ERR_ARG, "octave %d (%d .. %d)", octave, o.first_octave, o.first_octave + probe.n_octaves() - 1);
    }
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    SiftChunk ck(sg.s, o, width, height, channels);
    TRY(ck.alloc(1));
    TRY(ck.begin(image, 1));
    for (int q = 0; q < k; ++q) TRY(ck.next_octave());
    TRY(ck.detect());
    HIPCHK(hipStreamSynchronize(sg.s));
    const size_t npx = (size_t)ck.ow[(size_t)k] * ck.oh[(size_t)k];
    HIPCHK(ck.d_gauss.download(gauss, npx * (o.n_intervals + 3))); HIPCHK(ck.d_dog.download(dog, npx * (o.n_intervals + 2)));
    return LVBA_OK;
}

extern "C" int32_t lvba_sift_candidates(int32_t device, int32_t width, int32_t height, int32_t channels, const uint8_t *image,
                                        const lvba_sift_opts *opts, int64_t capacity, float *xys, int32_t *where, int64_t *count)
{
    if (!image || !count || capacity < 0 || (capacity > 0 && (!xys || !where))) return lvba_fail(LVBA_ERR_ARG, "null argument or capacity < 0");
    TRY(check_image(width, height, channels));
    lvba_sift_opts o;
    TRY(check_opts(opts, o));
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    SiftChunk ck(sg.s, o, width, height, channels);
    TRY(ck.alloc(1));
    TRY(ck.begin(image, 1));
    int64_t n = 0;
    for (int k = 0;; ++k) {
        TRY(ck.detect());
        if (ck.n_cand > 0) {
            std::vector<SiftCand> c((size_t)ck.n_cand);
            HIPCHK(hipStreamSynchronize(sg.s));
            HIPCHK(ck.d_cand.download(c.data(), c.size()));
            const double sc = ck.scale();
            for (const SiftCand &q : c) {
                if (!q.ok) continue;
                if (n < capacity) {
                    xys[3 * n] = (float)(((double)q.x + q.ox) * sc);
                    xys[3 * n + 1] = (float)(((double)q.y + q.oy) * sc);
                    xys[3 * n + 2] = (float)(q.sig * sc);
                    where[2 * n] = o.first_octave + k; where[2 * n + 1] = q.l;
                }
                ++n;
            }
        }
        if (k + 1 == ck.n_octaves()) break;
        TRY(ck.next_octave());
    }
    *count = n;
    return LVBA_OK;
}
