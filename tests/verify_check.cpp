// verify_check.cpp -- csrc/verify_device.h compiled for the host (tests/test_verify_host.py): the hypotheses of one pair formed the
// way verify_hypothesis_kernel forms them -- ransac_device.h' generator and sampler, the header's solvers and gate, one hypothesis
// after the other -- ransac_device.h' choice, and the refits with their sums taken in match order.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/verify_device.h"

using namespace lvba;

extern "C" {

// idx [H][k]
void emul_sample(uint64_t seed, int32_t lo, int32_t hi, int32_t H, int32_t m, int32_t k, int32_t *idx)
{
    for (int h = 0; h < H; ++h) {
        const uint64_t key = ransac_key(seed, lo, hi, h);
        if (k == 8) ransac_sample<8>(key, m, idx + 8 * (int64_t)h);
        else ransac_sample<2>(key, m, idx + 2 * (int64_t)h);
    }
}

void emul_relative_rotation(const double *Rlo, const double *Rhi, double *R) { verify_relative_rotation(Rlo, Rhi, R); }

// P [m][4] = (x_lo, y_lo, x_hi, y_hi); mask [m]
void emul_score(int32_t m, const double *P, const double *E, double tau2, uint8_t *mask)
{
    for (int i = 0; i < m; ++i) mask[i] = verify_inlier(E, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], tau2) ? 1 : 0;
}

static bool hypothesis(int method, uint64_t key, int32_t m, const double *P, const double *R, double *E)
{
    if (method == VERIFY_EIGHT_POINT) {
        int32_t idx[8];
        double A[72];
        ransac_sample<8>(key, m, idx);
        bool clean = true;
        for (int j = 0; j < 8; ++j) {
            const double *p = P + 4 * (int64_t)idx[j];
            clean &= verify_eight_row(A, 1, j, p[0], p[1], p[2], p[3]);
        }
        verify_zero(E);
        return clean && verify_eight_solve(A, 1, E);
    }
    int32_t idx[2];
    double p[8];
    ransac_sample<2>(key, m, idx);
    for (int j = 0; j < 2; ++j)
        for (int c = 0; c < 4; ++c) p[4 * j + c] = P[4 * (int64_t)idx[j] + c];
    return verify_known_rotation(p, R, E);
}

// E [H][9], count [H]; m >= k.  Returns the winner's h (-1: every hypothesis invalid).
int32_t emul_hypotheses(int32_t method, uint64_t seed, int32_t lo, int32_t hi, int32_t H, int32_t m, const double *P, const double *R,
                        double tau2, double *E, int32_t *count)
{
    for (int h = 0; h < H; ++h) {
        double *e = E + 9 * (int64_t)h;
        const bool valid = hypothesis(method, ransac_key(seed, lo, hi, h), m, P, R, e);
        int32_t c = 0;
        for (int i = 0; i < m; ++i) c += verify_inlier(e, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], tau2) ? 1 : 0;
        count[h] = valid ? c : -1;
    }
    return ransac_winner(H, [=](int32_t h) { return count[h]; }, [](int32_t h) { return h; });
}

// one refit of E over its inliers; returns 1 and the refit in F, or 0
int32_t emul_refit(int32_t method, int32_t m, const double *P, const double *R, double tau2, const double *E, double *F)
{
    for (int k = 0; k < 9; ++k) F[k] = E[k];
    if (method == VERIFY_EIGHT_POINT) {
        double N[81] = {}, V[81];
        for (int i = 0; i < m; ++i) {
            const double xl = P[4 * i], yl = P[4 * i + 1], xh = P[4 * i + 2], yh = P[4 * i + 3];
            if (!verify_inlier(E, xl, yl, xh, yh, tau2)) continue;
            const double a[9] = {xh * xl, xh * yl, xh, yh * xl, yh * yl, yh, xl, yl, 1.0};
            for (int r = 0; r < 9; ++r)
                for (int c = 0; c < 9; ++c) N[9 * r + c] += a[r] * a[c];
        }
        return verify_refit_eight(N, V, F) ? 1 : 0;
    }
    double C[6] = {};
    for (int i = 0; i < m; ++i) {
        const double xl = P[4 * i], yl = P[4 * i + 1], xh = P[4 * i + 2], yh = P[4 * i + 3];
        if (!verify_inlier(E, xl, yl, xh, yh, tau2)) continue;
        double c[3];
        verify_constraint(R, xl, yl, xh, yh, c);
        C[0] += c[0] * c[0]; C[1] += c[0] * c[1]; C[2] += c[0] * c[2]; C[3] += c[1] * c[1]; C[4] += c[1] * c[2]; C[5] += c[2] * c[2];
    }
    return verify_refit_rotation(C, R, F) ? 1 : 0;
}

int32_t emul_status(int32_t m, int32_t method, int32_t min_inliers, int32_t count)
{
    return ransac_status(m, verify_sample_size(method), min_inliers, count);
}

} // extern "C"
