// Host build of csrc/colorize_device.h (the colouriser's per-point rules, the code the kernels run) for
// tests/test_colorize_host.py, as a shared library bound with ctypes.  Built with -ffp-contract=off like colorize.hip.
#include <stdint.h>

#include "../global-lvba_amd/csrc/colorize_device.h"

using namespace lvba;

extern "C" {

// nseg pixel runs (zc[off[s] .. off[s+1])): kept flag and index of the winner inside the run
void emul_walks(int64_t nseg, const int64_t *off, const double *zc, uint8_t *kept, int64_t *win)
{
    for (int64_t s = 0; s < nseg; ++s) {
        const double *z = zc + off[s];
        int64_t w;
        kept[s] = col_walk(off[s + 1] - off[s], [&](int64_t q) { return z[q]; }, w) ? 1 : 0;
        win[s] = w;
    }
}

void emul_project(int64_t n, const float *pw, const double *R, const double *t, const double *intr, int W, int H, uint8_t *ok,
                  int64_t *pix, double *zc)
{
    const TrkIntr cam{intr[0], intr[1], intr[2], intr[3], intr[4], intr[5], intr[6], intr[7]};
    for (int64_t i = 0; i < n; ++i) {
        int64_t p = -1;
        double z = 0.0;
        ok[i] = col_project(cam, R, t, pw + 3 * i, W, H, p, z) ? 1 : 0;
        pix[i] = ok[i] ? p : -1;
        zc[i] = z;
    }
}

void emul_world(int64_t n, const float *pts, const double *T, float *out)
{
    for (int64_t i = 0; i < n; ++i) col_world_point(T, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], out + 3 * i);
}

void emul_leaf_key(int64_t n, const float *xyz, double leaf, int64_t *k, double *d2, uint8_t *ok)
{
    for (int64_t i = 0; i < n; ++i) ok[i] = col_leaf_key(xyz + 3 * i, leaf, k + 3 * i, d2[i]) ? 1 : 0;
}

void emul_window(int n, const double *t, double t_img, double half, int *lo_hi, uint8_t *in)
{
    col_window_range(t, n, t_img, half, lo_hi[0], lo_hi[1]);
    for (int i = 0; i < n; ++i) in[i] = col_in_window(t[i], t_img, half) ? 1 : 0;
}

} // extern "C"
