// sift_device.h -- scalar pieces of the SIFT extractor (sift.hip; the rule is in include/lvba_hip.h): the power of
// two of the scale, the fp64 refinement of a candidate, a sample of the orientation histogram and of the descriptor, the peak
// picking and the quantisation.  Host/device-neutral, like match_device.h: tests/sift_check.cpp runs them on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LVBA_SIFT_FN __host__ __device__ __forceinline__
#else
#define LVBA_SIFT_FN inline
#endif

namespace lvba {

constexpr int SIFT_TILE = 64;          // pixels of a row that one workgroup of the blur kernels covers
constexpr int SIFT_TILE_ROWS = 16;     // rows of a tile of the column blur
constexpr int SIFT_MAX_RADIUS = 32;    // largest blur radius (the halo of a tile)
constexpr int SIFT_MAX_INTERVALS = 5;
constexpr int SIFT_MAX_ORI = 4;        // largest max_orientations
constexpr int SIFT_ORI_BINS = 36;
constexpr int SIFT_DESC = 128;         // 4 x 4 x 8
constexpr int SIFT_MAX_MOVES = 5;
constexpr double SIFT_TWO_PI = 6.283185307179586;
constexpr double SIFT_LN2 = 0.6931471805599453;

// 2^z from + * / alone, so that the host and the device give the same bits: z = n + f with n = floor(z), 2^f = exp(f ln 2) as
// the Horner form of the first 21 terms of the series (f ln 2 < 0.7: the remainder is below 1e-20), then n exact doublings.
LVBA_SIFT_FN double sift_pow2(double z)
{
    int n = (int)z;
    if ((double)n > z) n -= 1;
    const double u = (z - (double)n) * SIFT_LN2;
    double r = 1.0;
    for (int k = 20; k >= 1; --k) r = 1.0 + (u / (double)k) * r;
    for (; n > 0; --n) r = r * 2.0;
    for (; n < 0; ++n) r = r * 0.5;
    return r;
}

// Refinement of the candidate (x, y, l) of one octave's DoG levels D [S + 2][h][w].  On success (x, y, l) is the sample the fit
// ended on and (ox, oy, ol) its offset, every component within 0.5.
LVBA_SIFT_FN bool sift_refine(const float *D, int w, int h, int S, double dog_threshold, double edge, int &x, int &y, int &l, double &ox,
                              double &oy, double &ol)
{
#define SIFT_D(L, Y, X) ((double)D[((int64_t)(L) * h + (Y)) * w + (X)])
    int moves = 0;
    double v, gx, gy, gs, dxx, dyy, dss, dxy, dxs, dys;
    for (;;) {
        v = SIFT_D(l, y, x);
        gx = 0.5 * (SIFT_D(l, y, x + 1) - SIFT_D(l, y, x - 1));
        gy = 0.5 * (SIFT_D(l, y + 1, x) - SIFT_D(l, y - 1, x));
        gs = 0.5 * (SIFT_D(l + 1, y, x) - SIFT_D(l - 1, y, x));
        dxx = (SIFT_D(l, y, x + 1) + SIFT_D(l, y, x - 1)) - 2.0 * v;
        dyy = (SIFT_D(l, y + 1, x) + SIFT_D(l, y - 1, x)) - 2.0 * v;
        dss = (SIFT_D(l + 1, y, x) + SIFT_D(l - 1, y, x)) - 2.0 * v;
        dxy = 0.25 * ((SIFT_D(l, y + 1, x + 1) - SIFT_D(l, y + 1, x - 1)) - (SIFT_D(l, y - 1, x + 1) - SIFT_D(l, y - 1, x - 1)));
        dxs = 0.25 * ((SIFT_D(l + 1, y, x + 1) - SIFT_D(l + 1, y, x - 1)) - (SIFT_D(l - 1, y, x + 1) - SIFT_D(l - 1, y, x - 1)));
        dys = 0.25 * ((SIFT_D(l + 1, y + 1, x) - SIFT_D(l + 1, y - 1, x)) - (SIFT_D(l - 1, y + 1, x) - SIFT_D(l - 1, y - 1, x)));
        // the adjugate of the symmetric Hessian [dxx dxy dxs; dxy dyy dys; dxs dys dss]
        const double c00 = dyy * dss - dys * dys, c01 = dxs * dys - dxy * dss, c02 = dxy * dys - dxs * dyy;
        const double c11 = dxx * dss - dxs * dxs, c12 = dxy * dxs - dxx * dys, c22 = dxx * dyy - dxy * dxy;
        const double det = (dxx * c00 + dxy * c01) + dxs * c02;
        if (det == 0.0) return false;
        ox = -(((c00 * gx + c01 * gy) + c02 * gs) / det);
        oy = -(((c01 * gx + c11 * gy) + c12 * gs) / det);
        ol = -(((c02 * gx + c12 * gy) + c22 * gs) / det);
        const bool sx = fabs(ox) <= 0.5, sy = fabs(oy) <= 0.5, sl = fabs(ol) <= 0.5;
        if (sx && sy && sl) break;
        if (moves == SIFT_MAX_MOVES) return false;
        ++moves;
        if (!sx) x += ox > 0.0 ? 1 : -1;
        if (!sy) y += oy > 0.0 ? 1 : -1;
        if (!sl) l += ol > 0.0 ? 1 : -1;
        if (x < 1 || x > w - 2 || y < 1 || y > h - 2 || l < 1 || l > S) return false;
    }
#undef SIFT_D
    const double contrast = v + 0.5 * ((gx * ox + gy * oy) + gs * ol);
    if (fabs(contrast) < dog_threshold / (double)S) return false;
    const double tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
    if (det2 <= 0.0) return false;
    if ((tr * tr) / det2 >= ((edge + 1.0) * (edge + 1.0)) / edge) return false;
    return true;
}

// the scale of a key point inside its octave: sigma0 2^((l + ol) / S); times 2^o it is the key point's sigma
LVBA_SIFT_FN double sift_octave_sigma(double sigma0, int S, int l, double ol) { return sigma0 * sift_pow2(((double)l + ol) / (double)S); }

// central differences of the Gaussian level G [h][w] at (px, py): false outside [1, w - 2] x [1, h - 2]
LVBA_SIFT_FN bool sift_gradient(const float *G, int w, int h, int px, int py, double &gx, double &gy)
{
    if (px < 1 || px > w - 2 || py < 1 || py > h - 2) return false;
    gx = (double)G[(int64_t)py * w + px + 1] - (double)G[(int64_t)py * w + px - 1];
    gy = (double)G[(int64_t)(py + 1) * w + px] - (double)G[(int64_t)(py - 1) * w + px];
    return true;
}

LVBA_SIFT_FN int sift_ori_radius(double window, double sig) { return (int)floor(window * (1.5 * sig) + 0.5); }

// sample (i, j) of the orientation window around the sample (x, y) with offset (ox, oy): its bin and weighted magnitude
LVBA_SIFT_FN bool sift_ori_sample(const float *G, int w, int h, int x, int y, int i, int j, int R, double ox, double oy, double sig, int &bin,
                                  double &val)
{
    if (i * i + j * j > R * R) return false;
    double gx, gy;
    if (!sift_gradient(G, w, h, x + i, y + j, gx, gy)) return false;
    const double ddx = (double)i - ox, ddy = (double)j - oy, s = 1.5 * sig;
    const double wgt = exp(-((ddx * ddx + ddy * ddy) / (2.0 * (s * s))));
    const double mag = sqrt(gx * gx + gy * gy);
    double a = atan2(gy, gx);
    if (a < 0.0) a = a + SIFT_TWO_PI;
    int b = (int)(a * ((double)SIFT_ORI_BINS / SIFT_TWO_PI));
    if (b >= SIFT_ORI_BINS) b = SIFT_ORI_BINS - 1;
    bin = b;
    val = mag * wgt;
    return true;
}

// hist [36] (smoothed in place, tmp [36] is scratch) -> the orientations, the larger peak first, a tie to the lower bin
LVBA_SIFT_FN int sift_ori_peaks(double *hist, double *tmp, int max_ori, double *theta)
{
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < SIFT_ORI_BINS; ++k)
            tmp[k] = ((hist[(k + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS] + hist[k]) + hist[(k + 1) % SIFT_ORI_BINS]) / 3.0;
        for (int k = 0; k < SIFT_ORI_BINS; ++k) hist[k] = tmp[k];
    }
    double top = 0.0;
    for (int k = 0; k < SIFT_ORI_BINS; ++k) top = hist[k] > top ? hist[k] : top;
    if (!(top > 0.0)) return 0;
    int n = 0;
    int pk[SIFT_MAX_ORI] = {0, 0, 0, 0};
    for (int k = 0; k < SIFT_ORI_BINS; ++k) {
        const double a = hist[(k + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS], b = hist[k], c = hist[(k + 1) % SIFT_ORI_BINS];
        if (!(b > a && b > c && b >= 0.8 * top)) continue;
        int at = n < max_ori ? n : max_ori; // insertion by descending value; equal values keep the lower bin in front
        while (at > 0 && hist[pk[at - 1]] < b) --at;
        if (at >= max_ori) continue;
        for (int m = (n < max_ori ? n : max_ori - 1); m > at; --m) pk[m] = pk[m - 1];
        pk[at] = k;
        if (n < max_ori) ++n;
    }
    for (int m = 0; m < n; ++m) {
        const int k = pk[m];
        const double a = hist[(k + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS], b = hist[k], c = hist[(k + 1) % SIFT_ORI_BINS];
        const double off = (0.5 * (a - c)) / ((a - 2.0 * b) + c);
        double t = (((double)k + 0.5) + off) * (SIFT_TWO_PI / (double)SIFT_ORI_BINS);
        if (t < 0.0) t = t + SIFT_TWO_PI;
        if (t >= SIFT_TWO_PI) t = t - SIFT_TWO_PI;
        theta[m] = t;
    }
    return n;
}

LVBA_SIFT_FN int sift_desc_radius(double sig) { return (int)floor((3.0 * sig) * 1.4142135623730951 * 2.5 + 0.5); }

// sample (i, j) of the descriptor window in the frame rotated by theta (ct, st its cosine and sine): the cell below it in the
// three directions, the fraction towards the next direction, and the weighted magnitude already shared among the four cells:
// p[2 dr + dc] = (v w_r) w_c, the first two factors of the rule's ((v w_r) w_c) w_o -- formed once by the lane that has the sample
struct SiftDescSample { int r0, c0, o0; double fo; double p[4]; };

LVBA_SIFT_FN bool sift_desc_sample(const float *G, int w, int h, int x, int y, int i, int j, double ox, double oy, double sig, double theta,
                                   double ct, double st, SiftDescSample &s)
{
    double gx, gy;
    if (!sift_gradient(G, w, h, x + i, y + j, gx, gy)) return false;
    const double ddx = (double)i - ox, ddy = (double)j - oy, hw = 3.0 * sig;
    const double rx = (ct * ddx + st * ddy) / hw, ry = (ct * ddy - st * ddx) / hw;
    const double cb = rx + 1.5, rb = ry + 1.5;
    if (!(rb > -1.0 && rb < 4.0 && cb > -1.0 && cb < 4.0)) return false;
    const double mag = sqrt(gx * gx + gy * gy);
    double a = atan2(gy, gx) - theta;
    if (a < 0.0) a = a + SIFT_TWO_PI;
    if (a < 0.0) a = a + SIFT_TWO_PI;
    if (a >= SIFT_TWO_PI) a = a - SIFT_TWO_PI;
    const double ob = a * (8.0 / SIFT_TWO_PI);
    const double wgt = exp(-((rx * rx + ry * ry) / 8.0));
    const double fr0 = floor(rb), fc0 = floor(cb), fo0 = floor(ob);
    s.r0 = (int)fr0; s.c0 = (int)fc0; s.o0 = (int)fo0 & 7;
    const double fr = rb - fr0, fc = cb - fc0, v = mag * wgt;
    const double v0 = v * (1.0 - fr), v1 = v * fr;
    s.p[0] = v0 * (1.0 - fc); s.p[1] = v0 * fc; s.p[2] = v1 * (1.0 - fc); s.p[3] = v1 * fc;
    s.fo = ob - fo0;
    return true;
}

// what the sample adds to the bin (r, c, o); false when nothing
LVBA_SIFT_FN bool sift_desc_share(const SiftDescSample &s, int r, int c, int o, double &add)
{
    const int dr = r - s.r0, dc = c - s.c0;
    if ((unsigned)dr > 1u || (unsigned)dc > 1u) return false;
    double wo;
    if (o == s.o0) wo = 1.0 - s.fo; else if (o == ((s.o0 + 1) & 7)) wo = s.fo; else return false;
    add = s.p[2 * dr + dc] * wo;
    return true;
}

// acc [128] (overwritten) -> the bytes: normalise, clamp at 0.2, normalise, 512 v rounded half up, at most 255; sums in bin order
LVBA_SIFT_FN void sift_desc_bytes(double *acc, uint8_t *out)
{
    double n2 = acc[0] * acc[0];
    for (int k = 1; k < SIFT_DESC; ++k) n2 = n2 + acc[k] * acc[k];
    if (!(n2 > 0.0)) {
        for (int k = 0; k < SIFT_DESC; ++k) out[k] = 0;
        return;
    }
    const double n = sqrt(n2);
    for (int k = 0; k < SIFT_DESC; ++k) {
        const double v = acc[k] / n;
        acc[k] = v > 0.2 ? 0.2 : v;
    }
    double m2 = acc[0] * acc[0];
    for (int k = 1; k < SIFT_DESC; ++k) m2 = m2 + acc[k] * acc[k];
    const double m = sqrt(m2);
    for (int k = 0; k < SIFT_DESC; ++k) {
        const double q = floor(512.0 * (acc[k] / m) + 0.5);
        out[k] = (uint8_t)(q > 255.0 ? 255.0 : q);
    }
}

} // namespace lvba
