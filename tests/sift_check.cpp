// sift_check.cpp -- csrc/sift_device.h on the host, walked as the kernels walk it: the refinement of a candidate, the orientation
// histogram with its peaks, the descriptor sums with their quantisation.  tests/test_sift_host.py builds it without contraction and
// compares it with the numpy oracle.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/sift_device.h"

using namespace lvba;

extern "C" {

double emul_pow2(double z) { return sift_pow2(z); }

// D [S + 2][h][w]; pos = (x, y, l) in and out; off = (ox, oy, ol); returns 1 when the key point stands
int emul_refine(const float *D, int w, int h, int S, double t, double e, int32_t *pos, double *off)
{
    int x = pos[0], y = pos[1], l = pos[2];
    const bool ok = sift_refine(D, w, h, S, t, e, x, y, l, off[0], off[1], off[2]);
    pos[0] = x; pos[1] = y; pos[2] = l;
    return ok ? 1 : 0;
}

// the histogram as sift_orient_kernel forms it: rounds of 64 samples, bin b summed by its own walk over each round
void emul_ori_hist(const float *G, int w, int h, int x, int y, double ox, double oy, double sig, double window, double *hist)
{
    const int R = sift_ori_radius(window, sig), side = 2 * R + 1, total = side * side;
    for (int b = 0; b < SIFT_ORI_BINS; ++b) hist[b] = 0.0;
    int s_bin[64];
    double s_val[64];
    for (int t0 = 0; t0 < total; t0 += 64) {
        for (int lane = 0; lane < 64; ++lane) {
            const int t = t0 + lane;
            int bin = -1;
            double val = 0.0;
            if (t < total && !sift_ori_sample(G, w, h, x, y, t % side - R, t / side - R, R, ox, oy, sig, bin, val)) bin = -1;
            s_bin[lane] = bin; s_val[lane] = val;
        }
        for (int b = 0; b < SIFT_ORI_BINS; ++b)
            for (int j = 0; j < 64; ++j)
                if (s_bin[j] == b) hist[b] = hist[b] + s_val[j];
    }
}

int emul_ori_peaks(const double *hist_in, int max_ori, double *theta)
{
    double hist[SIFT_ORI_BINS], tmp[SIFT_ORI_BINS];
    for (int b = 0; b < SIFT_ORI_BINS; ++b) hist[b] = hist_in[b];
    return sift_ori_peaks(hist, tmp, max_ori, theta);
}

// the 128 sums as sift_describe_kernel forms them: lane L owns the bins 2 L and 2 L + 1
void emul_desc_bins(const float *G, int w, int h, int x, int y, double ox, double oy, double sig, float theta_f, double *acc)
{
    const double theta = (double)theta_f, ct = cos(theta), st = sin(theta);
    const int R = sift_desc_radius(sig), side = 2 * R + 1, total = side * side;
    for (int k = 0; k < SIFT_DESC; ++k) acc[k] = 0.0;
    SiftDescSample smp[64];
    int s_ok[64];
    for (int t0 = 0; t0 < total; t0 += 64) {
        for (int lane = 0; lane < 64; ++lane) {
            const int t = t0 + lane;
            s_ok[lane] = t < total && sift_desc_sample(G, w, h, x, y, t % side - R, t / side - R, ox, oy, sig, theta, ct, st, smp[lane]);
        }
        for (int lane = 0; lane < 64; ++lane) {
            const int br = lane >> 4, bc = (lane >> 2) & 3, bo = 2 * (lane & 3);
            for (int j = 0; j < 64; ++j) {
                if (!s_ok[j]) continue;
                double add;
                if (sift_desc_share(smp[j], br, bc, bo, add)) acc[2 * lane] = acc[2 * lane] + add;
                if (sift_desc_share(smp[j], br, bc, bo + 1, add)) acc[2 * lane + 1] = acc[2 * lane + 1] + add;
            }
        }
    }
}

void emul_desc_bytes(const double *acc_in, uint8_t *out)
{
    double acc[SIFT_DESC];
    for (int k = 0; k < SIFT_DESC; ++k) acc[k] = acc_in[k];
    sift_desc_bytes(acc, out);
}

} // extern "C"
