// photo_check.cpp -- csrc/photo_device.h compiled for the host (tests/test_photo_host.py): the samples, the sums and the finish
// walked the way the kernels of photo.hip walk them, with the header's own functions.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include "../global-lvba_amd/csrc/photo_device.h"

using namespace lvba;

extern "C" {

// bounds: occlusion_rel, occlusion_abs, max_depth; flags: holes, min_views.  depth [M][h][w] or null; bgr [M][h][w][3].
// seen [M][n], c16 [M][n][3] (zeros where not sampled), n_views [n], s1 [n][3], s2 [n][3]: as photo_sample_kernel, a lane's point
// per iteration, the images in index order
void emul_sums(int64_t n, const float *xyz, int M, int w, int h, const float *depth, const double *Rcw, const double *tcw,
               const uint8_t *bgr, const double *intr, const double *bounds, const int32_t *flags, uint8_t *seen, int32_t *c16,
               int32_t *n_views, uint32_t *s1, int64_t *s2)
{
    const TrkIntr cam = trk_intr_of(intr);
    const PhotoRule o = photo_rule_of(depth != nullptr, bounds[0], bounds[1], bounds[2], flags[0], flags[1]);
    const int64_t npix = (int64_t)w * h;
    for (int64_t i = 0; i < n; ++i) {
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        PhotoSums acc{};
        for (int b = 0; b < M; ++b) {
            const uint8_t *img = bgr + 3 * npix * b;
            int32_t c[3] = {0, 0, 0};
            const bool hit = photo_sample(cam, depth ? depth + npix * b : nullptr, w, h, Rcw + 9 * (int64_t)b, tcw + 3 * (int64_t)b, X, o,
                                          [&](int y, int x) { return photo_texel_of(img + 3 * ((int64_t)y * w + x)); }, c);
            if (hit) photo_add(acc, c);
            seen[(int64_t)b * n + i] = hit ? 1 : 0;
            for (int k = 0; k < 3; ++k) c16[3 * ((int64_t)b * n + i) + k] = hit ? c[k] : 0;
        }
        n_views[i] = acc.n;
        for (int k = 0; k < 3; ++k) { s1[3 * i + k] = acc.s1[k]; s2[3 * i + k] = acc.s2[k]; }
    }
}

// the sums of one point after `times` views of the same sample
void emul_repeat(const int32_t *c16, int times, int32_t *n_views, uint32_t *s1, int64_t *s2)
{
    PhotoSums acc{};
    for (int k = 0; k < times; ++k) photo_add(acc, c16);
    *n_views = acc.n;
    for (int k = 0; k < 3; ++k) { s1[k] = acc.s1[k]; s2[k] = acc.s2[k]; }
}

// rgb [n][3], sigma [n]: as photo_finish_kernel
void emul_finish(int64_t n, const int32_t *n_views, const uint32_t *s1, const int64_t *s2, int min_views, uint8_t *rgb, double *sigma)
{
    for (int64_t i = 0; i < n; ++i) {
        PhotoSums s;
        s.n = n_views[i];
        for (int k = 0; k < 3; ++k) { s.s1[k] = s1[3 * i + k]; s.s2[k] = s2[3 * i + k]; }
        photo_rgb(s, rgb + 3 * i);
        sigma[i] = photo_sigma(s, min_views);
    }
}

} // extern "C"
