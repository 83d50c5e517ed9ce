// expo_device.h -- scalar pieces of the per-image exposure compensation (expo.hip, photo.hip; the rule is in include/lvba_hip.h,
// DESIGN.md §10r): the compensated sample, the decision whether a channel of a located sample is used, a point's terms of the 20
// estimation sums, and the solve with its gauge.  Host/device-neutral, like photo_device.h; tests/expo_check.cpp compiles it for
// the host.  Everything here is integer arithmetic; the only floating-point decisions are photo_locate's, unchanged.
//   Gains (A, B) per image and channel (b, g, r): A in units of 2^-16, B in units of 2^-16 of 1/256 grey level; identity (65536, 0).
//   c' = clamp(floor((A c16 + B + 32768) / 65536), 0, 65280) in int64: |A c16 + B| < 2^18 2^16 + 2^32 < 2^35.
//   Sums of an image (EXPO_NS = 20 uint64): per channel k at 6 k: n, sum c, sum ref, sum c^2, sum c ref, sum (c' - ref)^2 with
//   c = c16 raw; then n_located and the channel terms the gate refused.  With fewer than 2^32 points every sum is below
//   2^32 65280^2 < 2^64, because 65280^2 < 2^32.
#pragma once
#include <stdint.h>
#include "photo_device.h"

namespace lvba {

constexpr int EXPO_NS = 20;                 // sums per image
constexpr int EXPO_PER = 6;                 // sums per channel: n, sum c, sum ref, sum c^2, sum c ref, sum (c' - ref)^2
constexpr int EXPO_LOCATED = 18, EXPO_REFUSED = 19;
constexpr int EXPO_BLOCK = 256;             // lanes of a sums workgroup
constexpr int EXPO_CHUNK = 4096;            // points of a workgroup: lane l takes the points chunk * EXPO_CHUNK + l + k * EXPO_BLOCK
constexpr int64_t EXPO_ONE = 65536;         // the gain 1
constexpr int64_t EXPO_A_MIN = (int64_t)1 << 14, EXPO_A_MAX = (int64_t)1 << 18; // the gains an entry point takes: 1/4 .. 4
constexpr int64_t EXPO_B_MAX = (int64_t)65536 * 65280;                          // and |B|: the whole range of a sample
constexpr int32_t EXPO_C_MAX = 65280;
// image states (the LVBA_EXPO_* values of include/lvba_hip.h), ordered: an image's state is the largest of its channels'
enum { EXPO_OK = 0, EXPO_FALLBACK_GAIN = 1, EXPO_TOO_FEW = 2, EXPO_OUT_OF_BOUNDS = 3 };
enum { EXPO_AFFINE = 0, EXPO_GAIN = 1 };    // LVBA_EXPO_AFFINE, LVBA_EXPO_GAIN

struct ExpoRule { int32_t sat_lo, sat_hi, gate16, pad; }; // gate16 = gate * 256, 0: off

// the number of workgroups the n points of an image are summed by: a function of n alone
LVBA_TRK_FN int64_t expo_chunks(int64_t n) { return n <= EXPO_CHUNK ? 1 : (n + EXPO_CHUNK - 1) / EXPO_CHUNK; }

// floor(a / b), b > 0: C++ truncates towards zero, Python's // floors; the remainder's sign tells the two apart
template <class I>
LVBA_TRK_FN I expo_floor_div(I a, I b)
{
    const I q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

// the compensated sample
LVBA_TRK_FN int32_t expo_apply(int64_t A, int64_t B, int32_t c16)
{
    const int64_t q = expo_floor_div<int64_t>(A * (int64_t)c16 + B + 32768, EXPO_ONE);
    return (int32_t)(q < 0 ? 0 : (q > EXPO_C_MAX ? EXPO_C_MAX : q));
}

// are the n (A, B) pairs gains an entry point takes?
LVBA_TRK_FN bool expo_gains_ok(const int64_t *g, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) {
        const int64_t A = g[2 * i], B = g[2 * i + 1];
        if (A < EXPO_A_MIN || A > EXPO_A_MAX || B < -EXPO_B_MAX || B > EXPO_B_MAX) return false;
    }
    return true;
}

// are the four texel bytes of channel k all in [sat_lo, sat_hi]?  A clipped texel breaks the affine model.
LVBA_TRK_FN bool expo_unsaturated(const PhotoTap &p, int k, const ExpoRule &e)
{
    const uint32_t t[4] = {p.t00, p.t10, p.t01, p.t11};
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int32_t v = photo_byte(t[q], k);
        ok = ok && v >= e.sat_lo && v <= e.sat_hi;
    }
    return ok;
}

// A lane's share of an image's sums: at most EXPO_CHUNK / EXPO_BLOCK = 16 points, so the counts and the first-order sums fit 32
// bits (16 65280 < 2^21; a whole workgroup's 4096 65280 < 2^29); the products take 64.
struct ExpoAcc {
    uint32_t n[3], sc[3], sr[3];
    uint64_t scc[3], scr[3], see[3];
    uint32_t located, refused;
};

LVBA_TRK_FN void expo_acc_zero(ExpoAcc &a)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.n[k] = a.sc[k] = a.sr[k] = 0u; a.scc[k] = a.scr[k] = a.see[k] = 0u; }
    a.located = a.refused = 0u;
}

// channel k of a located sample into the sums: c16 raw, ref the reference, (A, B) the gains the gate and the residual are taken under
LVBA_TRK_FN void expo_channel(const PhotoTap &p, int k, int32_t ref, int64_t A, int64_t B, const ExpoRule &e, ExpoAcc &a)
{
    if (!expo_unsaturated(p, k, e)) return;
    const int32_t c = photo_mix_channel(p, k);
    const int32_t d = expo_apply(A, B, c) - ref;
    if (e.gate16 > 0 && (d > e.gate16 || -d > e.gate16)) { a.refused += 1u; return; }
    a.n[k] += 1u;
    a.sc[k] += (uint32_t)c;
    a.sr[k] += (uint32_t)ref;
    a.scc[k] += (uint64_t)((int64_t)c * c);
    a.scr[k] += (uint64_t)((int64_t)c * ref);
    a.see[k] += (uint64_t)((int64_t)d * d);
}

// One valid point in one image: located exactly as the fusion locates it, then its three channels.  gains [3][2] of the image.
template <class Texel>
LVBA_TRK_FN void expo_point(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                            const double *__restrict__ tj, const double *__restrict__ X, const uint16_t *__restrict__ ref16,
                            const PhotoRule &o, const ExpoRule &e, const int64_t *__restrict__ gains, Texel texel, ExpoAcc &a)
{
    double u, v;
    if (!photo_locate(cam, depth_j, w, h, Rj, tj, X, o, u, v)) return;
    const PhotoTap p = photo_tap(u, v, texel);
    a.located += 1u;
#pragma unroll
    for (int k = 0; k < 3; ++k) expo_channel(p, k, (int32_t)ref16[k], gains[2 * k], gains[2 * k + 1], e, a);
}

// the share as the 20 sums, added to s
LVBA_TRK_FN void expo_acc_add(const ExpoAcc &a, uint64_t *__restrict__ s)
{
    for (int k = 0; k < 3; ++k) {
        uint64_t *q = s + EXPO_PER * k;
        q[0] += a.n[k]; q[1] += a.sc[k]; q[2] += a.sr[k]; q[3] += a.scc[k]; q[4] += a.scr[k]; q[5] += a.see[k];
    }
    s[EXPO_LOCATED] += a.located; s[EXPO_REFUSED] += a.refused;
}

// ---- the solve and the gauge: host functions, integers throughout, 128 bits where a product needs them ---------------------------
typedef __int128 expo_i128;

struct ExpoSolveRule { // lvba_expo_opts as integers
    int32_t model, min_samples, min_spread, pad;
    int64_t a_lo, a_hi, b_max; // min_gain, max_gain in units of 2^-16; max_offset in units of 2^-16 of 1/256 grey level
};

// the gain-only form A = floor((sum c ref 2^16 + sum c^2 / 2) / sum c^2); false where sum c^2 = 0
inline bool expo_gain_only(uint64_t scc, uint64_t scr, expo_i128 &A)
{
    if (scc == 0) return false;
    A = expo_floor_div<expo_i128>((expo_i128)scr * EXPO_ONE + (expo_i128)(scc / 2), (expo_i128)scc);
    return true;
}

// one channel from its six sums: the state, and (A, B) where the state is OK or FALLBACK_GAIN
inline int expo_solve_channel(const uint64_t *s, const ExpoSolveRule &o, int64_t &Aout, int64_t &Bout)
{
    const uint64_t n = s[0], sc = s[1], sr = s[2], scc = s[3], scr = s[4];
    Aout = EXPO_ONE; Bout = 0;
    if (n < (uint64_t)o.min_samples) return EXPO_TOO_FEW;
    int state = EXPO_OK;
    expo_i128 A, B = 0;
    bool affine = o.model == EXPO_AFFINE;
    const expo_i128 D = (expo_i128)n * scc - (expo_i128)sc * sc;
    if (affine) {
        const expo_i128 flat = (expo_i128)n * n * ((expo_i128)o.min_spread * 256 * o.min_spread * 256);
        if (D <= flat) { affine = false; state = EXPO_FALLBACK_GAIN; } // too flat to tell a gain from an offset
    }
    if (affine) {
        const expo_i128 N = (expo_i128)n * scr - (expo_i128)sc * sr;
        A = expo_floor_div<expo_i128>(N * EXPO_ONE + D / 2, D);
    } else if (!expo_gain_only(scc, scr, A)) {
        return EXPO_OUT_OF_BOUNDS; // every used sample is black: no gain explains the reference
    }
    if (A < o.a_lo || A > o.a_hi) return EXPO_OUT_OF_BOUNDS; // (before B: a wild A would not fit the product below)
    if (affine) {
        B = expo_floor_div<expo_i128>(((expo_i128)sr * EXPO_ONE - A * sc) * 2 + n, (expo_i128)2 * n);
        if (B < -(expo_i128)o.b_max || B > (expo_i128)o.b_max) return EXPO_OUT_OF_BOUNDS;
    }
    Aout = (int64_t)A; Bout = (int64_t)B;
    return state;
}

// gains [n_images][3][2], status [n_images] from sums [n_images][EXPO_NS]: per image the worst of its channels, identity on all
// three where that is TOO_FEW or OUT_OF_BOUNDS; then the gauge per channel over the images that are OK or FALLBACK_GAIN -- mean
// gain 1, mean offset 0 --; an image whose gauged gains an entry point would refuse becomes OUT_OF_BOUNDS with identity.
inline void expo_solve(int64_t n_images, const uint64_t *sums, const ExpoSolveRule &o, int64_t *gains, int32_t *status)
{
    for (int64_t j = 0; j < n_images; ++j) {
        int st = EXPO_OK;
        for (int k = 0; k < 3; ++k) {
            const int sk = expo_solve_channel(sums + EXPO_NS * j + EXPO_PER * k, o, gains[6 * j + 2 * k], gains[6 * j + 2 * k + 1]);
            st = sk > st ? sk : st;
        }
        status[j] = st;
        if (st >= EXPO_TOO_FEW)
            for (int k = 0; k < 3; ++k) { gains[6 * j + 2 * k] = EXPO_ONE; gains[6 * j + 2 * k + 1] = 0; }
    }
    for (int k = 0; k < 3; ++k) {
        int64_t n_ok = 0, sumA = 0;
        for (int64_t j = 0; j < n_images; ++j)
            if (status[j] <= EXPO_FALLBACK_GAIN) { n_ok += 1; sumA += gains[6 * j + 2 * k]; }
        if (n_ok == 0) continue;
        const int64_t S = expo_floor_div<int64_t>(n_ok * ((int64_t)1 << 32) + sumA / 2, sumA); // <= 2^18: A >= 2^14
        int64_t sumB = 0;
        for (int64_t j = 0; j < n_images; ++j)
            if (status[j] <= EXPO_FALLBACK_GAIN) {
                int64_t &A = gains[6 * j + 2 * k], &B = gains[6 * j + 2 * k + 1];
                A = expo_floor_div<int64_t>(A * S + 32768, EXPO_ONE);
                B = expo_floor_div<int64_t>(B * S + 32768, EXPO_ONE); // |B S| < 2^33 2^18
                sumB += B;
            }
        const int64_t T = expo_floor_div<int64_t>(2 * sumB + n_ok, 2 * n_ok); // the round-half-up mean
        for (int64_t j = 0; j < n_images; ++j)
            if (status[j] <= EXPO_FALLBACK_GAIN) gains[6 * j + 2 * k + 1] -= T;
    }
    for (int64_t j = 0; j < n_images; ++j)
        if (status[j] <= EXPO_FALLBACK_GAIN && !expo_gains_ok(gains + 6 * j, 3)) {
            status[j] = EXPO_OUT_OF_BOUNDS;
            for (int k = 0; k < 3; ++k) { gains[6 * j + 2 * k] = EXPO_ONE; gains[6 * j + 2 * k + 1] = 0; }
        }
}

} // namespace lvba
