// expo_check.cpp -- csrc/expo_device.h compiled for the host (tests/test_expo_host.py): the compensated sample, the estimation
// sums walked the way expo_sums_kernel walks them (a lane's share in the header's own 32- and 64-bit counters), the fusion with
// gains as photo_sample_kernel's gains instantiation adds it, and the solve with its gauge.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include "../global-lvba_amd/csrc/expo_device.h"

using namespace lvba;

extern "C" {

void emul_apply(int64_t n, int64_t A, int64_t B, const int32_t *c16, int32_t *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = expo_apply(A, B, c16[i]);
}

// bounds: occlusion_rel, occlusion_abs, max_depth; flags: holes, sat_lo, sat_hi, gate.  depth [M][h][w] or null; bgr [M][h][w][3];
// gains [M][3][2] or null (identity).  sums [M][20]
void emul_sums(int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int M, int w, int h, const float *depth,
               const double *Rcw, const double *tcw, const uint8_t *bgr, const double *intr, const double *bounds, const int32_t *flags,
               const int64_t *gains, uint64_t *sums)
{
    const TrkIntr cam = trk_intr_of(intr);
    const PhotoRule o = photo_rule_of(depth != nullptr, bounds[0], bounds[1], bounds[2], flags[0], 2);
    const ExpoRule e{flags[1], flags[2], flags[3] * 256, 0};
    const int64_t npix = (int64_t)w * h;
    const int64_t identity[6] = {EXPO_ONE, 0, EXPO_ONE, 0, EXPO_ONE, 0};
    for (int j = 0; j < M; ++j) {
        const uint8_t *img = bgr + 3 * npix * j;
        uint64_t *s = sums + EXPO_NS * (int64_t)j;
        for (int q = 0; q < EXPO_NS; ++q) s[q] = 0;
        for (int64_t chunk = 0; chunk < expo_chunks(n); ++chunk)
            for (int lane = 0; lane < EXPO_BLOCK; ++lane) {
                ExpoAcc acc;
                expo_acc_zero(acc);
                for (int k = 0; k < EXPO_CHUNK / EXPO_BLOCK; ++k) {
                    const int64_t i = chunk * EXPO_CHUNK + lane + (int64_t)k * EXPO_BLOCK;
                    if (i >= n) break;
                    if (!valid[i]) continue;
                    const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
                    expo_point(cam, depth ? depth + npix * j : nullptr, w, h, Rcw + 9 * (int64_t)j, tcw + 3 * (int64_t)j, X, ref16 + 3 * i, o, e,
                               gains ? gains + 6 * (int64_t)j : identity,
                               [&](int y, int x) { return photo_texel_of(img + 3 * ((int64_t)y * w + x)); }, acc);
                }
                expo_acc_add(acc, s);
            }
    }
}

// the fusion's sums with gains [M][3][2]: bounds as above; flags: holes
void emul_fuse(int64_t n, const float *xyz, int M, int w, int h, const float *depth, const double *Rcw, const double *tcw, const uint8_t *bgr,
               const double *intr, const double *bounds, const int32_t *flags, const int64_t *gains, int32_t *n_views, uint32_t *s1,
               int64_t *s2)
{
    const TrkIntr cam = trk_intr_of(intr);
    const PhotoRule o = photo_rule_of(depth != nullptr, bounds[0], bounds[1], bounds[2], flags[0], 2);
    const int64_t npix = (int64_t)w * h;
    for (int64_t i = 0; i < n; ++i) {
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        PhotoSums acc{};
        for (int b = 0; b < M; ++b) {
            const uint8_t *img = bgr + 3 * npix * b;
            int32_t c[3] = {0, 0, 0};
            if (!photo_sample(cam, depth ? depth + npix * b : nullptr, w, h, Rcw + 9 * (int64_t)b, tcw + 3 * (int64_t)b, X, o,
                              [&](int y, int x) { return photo_texel_of(img + 3 * ((int64_t)y * w + x)); }, c))
                continue;
            const int64_t *g = gains + 6 * (int64_t)b;
            for (int k = 0; k < 3; ++k) c[k] = expo_apply(g[2 * k], g[2 * k + 1], c[k]);
            photo_add(acc, c);
        }
        n_views[i] = acc.n;
        for (int k = 0; k < 3; ++k) { s1[3 * i + k] = acc.s1[k]; s2[3 * i + k] = acc.s2[k]; }
    }
}

// ints: model, min_samples, min_spread; lims: a_lo, a_hi, b_max
void emul_solve(int64_t n_images, const uint64_t *sums, const int32_t *ints, const int64_t *lims, int64_t *gains, int32_t *status)
{
    const ExpoSolveRule r{ints[0], ints[1], ints[2], 0, lims[0], lims[1], lims[2]};
    expo_solve(n_images, sums, r, gains, status);
}

int emul_gains_ok(const int64_t *g, int64_t n) { return expo_gains_ok(g, n) ? 1 : 0; }

} // extern "C"
