// verify_h_check.cpp -- the homography pieces of csrc/verify_device.h compiled for the host (tests/test_verify_h_host.py): the
// hypotheses of one pair formed the way verify_hypothesis_kernel<VERIFY_HOMOGRAPHY> forms them -- ransac_device.h' generator and
// sampler, the rows, verify_eight_solve, the sign, the inverse direction, the transfer gate, one hypothesis after the other --
// ransac_device.h' choice, the refit with its sums taken in match order, and the E-or-H decision.  TEST INFRASTRUCTURE ONLY.
// With -DVERIFY_H_MAIN it is a stand-alone program over the same functions, for a build under the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../global-lvba_amd/csrc/verify_device.h"

using namespace lvba;

extern "C" {

// P [m][4] = (x_lo, y_lo, x_hi, y_hi); mask [m].  All 0 where H has no inverse direction.
void emul_h_score(int32_t m, const double *P, const double *H, double tau2, uint8_t *mask)
{
    double G[9];
    const bool ok = verify_homography_inverse(H, G);
    for (int i = 0; i < m; ++i) mask[i] = ok && verify_inlier_h(H, G, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], tau2) ? 1 : 0;
}

// H, G [Hn][9], count [Hn]; m >= 4.  Returns the winner's h (-1: every hypothesis invalid).
int32_t emul_h_hypotheses(uint64_t seed, int32_t lo, int32_t hi, int32_t Hn, int32_t m, const double *P, double tau2, double *H, double *G,
                          int32_t *count)
{
    for (int h = 0; h < Hn; ++h) {
        double *e = H + 9 * (int64_t)h, *g = G + 9 * (int64_t)h;
        int32_t idx[4];
        double A[72];
        ransac_sample<4>(ransac_key(seed, lo, hi, h), m, idx);
        bool clean = true;
        for (int j = 0; j < 4; ++j) {
            const double *p = P + 4 * (int64_t)idx[j];
            clean &= verify_homography_rows(A, 1, j, p[0], p[1], p[2], p[3]);
        }
        verify_zero(e);
        verify_zero(g);
        const double *p0 = P + 4 * (int64_t)idx[0];
        const bool valid = clean && verify_homography_solve(A, 1, p0[0], p0[1], e, g);
        int32_t c = 0;
        for (int i = 0; i < m; ++i) c += verify_inlier_h(e, g, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], tau2) ? 1 : 0;
        count[h] = valid ? c : -1;
    }
    return ransac_winner(Hn, [=](int32_t h) { return count[h]; }, [](int32_t h) { return h; });
}

// one refit of H over its inliers; returns 1 and the refit in F, or 0
int32_t emul_h_refit(int32_t m, const double *P, double tau2, const double *H, double *F)
{
    double G[9], N[81] = {}, V[81];
    for (int k = 0; k < 9; ++k) F[k] = H[k];
    if (!verify_homography_inverse(H, G)) return 0;
    for (int i = 0; i < m; ++i) {
        const double xl = P[4 * i], yl = P[4 * i + 1], xh = P[4 * i + 2], yh = P[4 * i + 3];
        if (!verify_inlier_h(H, G, xl, yl, xh, yh, tau2)) continue;
        double r1[9], r2[9];
        verify_homography_row_pair(xl, yl, xh, yh, r1, r2);
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) N[9 * r + c] += r1[r] * r1[c] + r2[r] * r2[c];
    }
    return verify_refit_homography(N, V, F, G) ? 1 : 0;
}

int32_t emul_h_status(int32_t m, int32_t min_inliers, int32_t count) { return ransac_status(m, verify_sample_size(VERIFY_HOMOGRAPHY), min_inliers, count); }

int32_t emul_h_choose(int32_t status_E, int32_t n_E, int32_t status_H, int32_t n_H, double planar_ratio)
{
    return verify_choose_model(status_E, n_E, status_H, n_H, planar_ratio);
}

} // extern "C"

#ifdef VERIFY_H_MAIN
// A plane seen by two cameras, 40 matches of which every fourth is wrong, plus a NaN point: hypotheses, refit, score, choice.
int main()
{
    const int m = 41, Hn = 130;
    const double Ht[9] = {0.98, 0.03, 0.11, -0.02, 1.01, -0.07, 0.05, -0.04, 1.0};
    std::vector<double> P(4 * m);
    uint64_t z = 12345;
    auto rnd = [&z]() { z = ransac_mix(z + RANSAC_GOLDEN); return (double)(z >> 11) / 9007199254740992.0 - 0.5; };
    for (int i = 0; i < m; ++i) {
        const double x = rnd(), y = 0.8 * rnd(), w = (Ht[6] * x + Ht[7] * y) + Ht[8];
        P[4 * i] = x; P[4 * i + 1] = y;
        P[4 * i + 2] = ((Ht[0] * x + Ht[1] * y) + Ht[2]) / w + (i % 4 == 3 ? 0.2 + 0.1 * rnd() : 1e-4 * rnd());
        P[4 * i + 3] = ((Ht[3] * x + Ht[4] * y) + Ht[5]) / w + (i % 4 == 3 ? -0.15 : 1e-4 * rnd());
    }
    P[4 * (m - 1)] = NAN;
    const double tau2 = 1e-4;
    std::vector<double> H(9 * Hn), G(9 * Hn);
    std::vector<int32_t> count(Hn);
    const int32_t win = emul_h_hypotheses(7, 0, 1, Hn, m, P.data(), tau2, H.data(), G.data(), count.data());
    if (win < 0) { std::printf("no winner\n"); return 1; }
    double F[9];
    const int32_t ok = emul_h_refit(m, P.data(), tau2, H.data() + 9 * win, F);
    std::vector<uint8_t> mask(m);
    emul_h_score(m, P.data(), ok ? F : H.data() + 9 * win, tau2, mask.data());
    int n = 0, wrong = 0;
    for (int i = 0; i < m; ++i) { n += mask[i]; wrong += mask[i] && (i % 4 == 3 || i == m - 1); }
    const int kind = emul_h_choose(RANSAC_OK, n + 3, emul_h_status(m, 15, n), n, VERIFY_PLANAR_RATIO);
    std::printf("winner %d count %d refit %d inliers %d wrong %d kind %d\n", win, count[win], ok, n, wrong, kind);
    return n == 30 && wrong == 0 && kind == VERIFY_MODEL_HOMOGRAPHY ? 0 : 1;
}
#endif
