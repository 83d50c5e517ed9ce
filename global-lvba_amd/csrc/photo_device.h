// photo_device.h -- scalar pieces of the multi-view colour fusion (photo.hip; the rule is in include/lvba_hip.h):
// the sample of a point in an image -- covis_fate unchanged, then integer arithmetic on four texels -- and the finish of a point
// from its integer sums.  Host/device-neutral, like covis_device.h; tests/photo_check.cpp compiles it for the host.
#pragma once
#include <math.h>
#include <stdint.h>
#include "covis_device.h"

namespace lvba {

constexpr int PHOTO_MAX_IMAGES = 32768; // S1 <= 32 768 * 65 280 < 2^31, n S2 - S1^2 <= 4.6e18 < 2^63

struct PhotoRule {
    CovisRule covis;  // occlusion (a depth set was given), occlusion_rel, occlusion_abs; the rest unused
    double max_depth; // 0: none
    int32_t holes, min_views;
};

LVBA_TRK_FN PhotoRule photo_rule_of(bool occlusion, double occlusion_rel, double occlusion_abs, double max_depth, int32_t holes,
                                    int32_t min_views)
{
    PhotoRule r;
    r.covis = CovisRule{occlusion ? 1 : 0, 0, 0, 0, 0.0, occlusion_rel, occlusion_abs};
    r.max_depth = max_depth; r.holes = holes; r.min_views = min_views;
    return r;
}

// A texel as one word: b | g << 8 | r << 16 (the image's channel order from the low byte up), from its three bytes as uploaded.
LVBA_TRK_FN uint32_t photo_texel_of(const uint8_t *__restrict__ bgr) { return (uint32_t)bgr[0] | ((uint32_t)bgr[1] << 8) | ((uint32_t)bgr[2] << 16); }

// Where X is sampled in image j: false where the point is not sampled; else the projection's doubles (u, v), 0 <= u < w - 1,
// 0 <= v < h - 1.  depth_j may be null when the rule has no occlusion test.
LVBA_TRK_FN bool photo_locate(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                              const double *__restrict__ tj, const double *__restrict__ X, const PhotoRule &o, double &u, double &v)
{
    if (!(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]))) return false;
    const int fate = covis_fate(cam, depth_j, w, h, Rj, tj, X, o.covis);
    if (!(fate == COVIS_SEEN || (fate == COVIS_SEEN_HOLE && o.holes != 0))) return false;
    if (o.max_depth > 0.0) {
        const double Z = Rj[6] * X[0] + Rj[7] * X[1] + Rj[8] * X[2] + tj[2]; // the expression covis_fate evaluates
        if (!(Z <= o.max_depth)) return false;
    }
    return trk_project(cam, Rj, tj, X, u, v); // the same doubles as inside covis_fate
}

// The four texels about (u, v) and their 1/256-pixel fractions: texel(y, x) returns the word of pixel (y, x); t00 = (y, x),
// t10 = (y, x + 1), t01 = (y + 1, x), t11 = (y + 1, x + 1) with x = floor(u), y = floor(v)
struct PhotoTap { int32_t a, b; uint32_t t00, t10, t01, t11; };

template <class Texel>
LVBA_TRK_FN PhotoTap photo_tap(double u, double v, Texel texel)
{
    const double xf = floor(u), yf = floor(v);
    const int x = (int)xf, y = (int)yf;
    PhotoTap p;
    p.a = (int32_t)floor((u - xf) * 256.0); p.b = (int32_t)floor((v - yf) * 256.0); // exact: 0 .. 255
    p.t00 = texel(y, x); p.t10 = texel(y, x + 1); p.t01 = texel(y + 1, x); p.t11 = texel(y + 1, x + 1);
    return p;
}

// byte k (0 b, 1 g, 2 r) of a texel word
LVBA_TRK_FN int32_t photo_byte(uint32_t t, int k) { return (int32_t)((t >> (8 * k)) & 255u); }

// channel k of the bilinear mix of the tap's texels, in units of 1/256 grey level
LVBA_TRK_FN int32_t photo_mix_channel(const PhotoTap &p, int k)
{
    const int32_t a = p.a, b = p.b;
    const int32_t w00 = (256 - a) * (256 - b), w10 = a * (256 - b), w01 = (256 - a) * b, w11 = a * b;
    const int32_t c = w00 * photo_byte(p.t00, k) + w10 * photo_byte(p.t10, k) + w01 * photo_byte(p.t01, k) +
                      w11 * photo_byte(p.t11, k); // <= 255 * 65 536
    return (c + 128) >> 8;                        // <= 65 280
}

// c16 [3] (b, g, r)
LVBA_TRK_FN void photo_mix(const PhotoTap &p, int32_t *__restrict__ c16)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) c16[k] = photo_mix_channel(p, k);
}

// The sample of X in image j: false where the point is not sampled; else c16 [3] (b, g, r) in units of 1/256 grey level.
template <class Texel>
LVBA_TRK_FN bool photo_sample(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                              const double *__restrict__ tj, const double *__restrict__ X, const PhotoRule &o, Texel texel,
                              int32_t *__restrict__ c16)
{
    double u, v;
    if (!photo_locate(cam, depth_j, w, h, Rj, tj, X, o, u, v)) return false;
    photo_mix(photo_tap(u, v, texel), c16);
    return true;
}

// The running sums of a point: n views, s1 = sum c16, s2 = sum c16^2, channels b, g, r
struct PhotoSums { int32_t n; uint32_t s1[3]; int64_t s2[3]; };

LVBA_TRK_FN void photo_add(PhotoSums &s, const int32_t *__restrict__ c16)
{
    s.n += 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { s.s1[k] += (uint32_t)c16[k]; s.s2[k] += (int64_t)c16[k] * (int64_t)c16[k]; }
}

// rgb [3] = r, g, b: the round-half-up mean per channel, 0 0 0 without a view
LVBA_TRK_FN void photo_rgb(const PhotoSums &s, uint8_t *__restrict__ rgb)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t n = s.n;
        rgb[2 - k] = n > 0 ? (uint8_t)((2 * (int64_t)s.s1[k] + 256 * n) / (512 * n)) : (uint8_t)0;
    }
}

// the RMS over the channels of the per-channel standard deviation across the views, in grey levels; NaN below min_views (>= 2)
LVBA_TRK_FN double photo_sigma(const PhotoSums &s, int32_t min_views)
{
    if (s.n < min_views) return NAN;
    const int64_t n = s.n;
    int64_t N[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) N[k] = n * s.s2[k] - (int64_t)s.s1[k] * (int64_t)s.s1[k]; // exact, >= 0
    return sqrt((((double)N[0] + (double)N[1]) + (double)N[2]) / (3.0 * 65536.0 * (double)(n * n)));
}

} // namespace lvba
