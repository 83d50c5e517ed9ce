// resect_check.cpp -- csrc/resect_device.h compiled for the host (tests/test_resect_host.py): the hypotheses of one job formed the
// way resect_hypothesis_kernel forms them -- the sampler of ransac_device.h keyed on (seed, id, -1, h), the minimal solver, the
// inlier test, one hypothesis after the other -- ransac_device.h' choice, and the refinement rounds with their sums taken in correspondence
// order.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/resect_device.h"

using namespace lvba;

extern "C" {

// rec [m][5] from xy [m][2] (NaN: not undistorted) and world [m][3]
void emul_pack(int32_t m, const double *xy, const double *world, double *rec)
{
    for (int i = 0; i < m; ++i) resect_pack(xy[2 * i], xy[2 * i + 1], world + 3 * (int64_t)i, rec + RESECT_REC * (int64_t)i);
}

// idx [H][4]
void emul_sample(uint64_t seed, int32_t id, int32_t H, int32_t m, int32_t *idx)
{
    for (int h = 0; h < H; ++h) ransac_sample<RESECT_K>(ransac_key(seed, id, -1, h), m, idx + RESECT_K * (int64_t)h);
}

// the minimal solver on four records given directly; returns 1 and (R, t), or 0
int32_t emul_p3p(const double *c, double fx, double fy, double *R, double *t)
{
    return resect_p3p(c, c + RESECT_REC, c + 2 * RESECT_REC, c + 3 * RESECT_REC, fx, fy, R, t) ? 1 : 0;
}

void emul_score(int32_t m, const double *rec, const double *R, const double *t, double fx, double fy, double rho, uint8_t *mask)
{
    for (int i = 0; i < m; ++i) {
        const double *c = rec + RESECT_REC * (int64_t)i;
        mask[i] = resect_inlier(R, t, fx, fy, rho, c[0], c[1], c[2], c[3], c[4]) ? 1 : 0;
    }
}

// R [H][9], t [H][3], count [H]; m >= 4.  Returns the winner's h (-1: every hypothesis invalid).
int32_t emul_hypotheses(uint64_t seed, int32_t id, int32_t H, int32_t m, const double *rec, double fx, double fy, double rho, double *R, double *t,
                        int32_t *count)
{
    for (int h = 0; h < H; ++h) {
        int32_t idx[RESECT_K];
        ransac_sample<RESECT_K>(ransac_key(seed, id, -1, h), m, idx);
        double *r = R + 9 * (int64_t)h, *tt = t + 3 * (int64_t)h;
        const bool valid = resect_p3p(rec + RESECT_REC * (int64_t)idx[0], rec + RESECT_REC * (int64_t)idx[1], rec + RESECT_REC * (int64_t)idx[2],
                                      rec + RESECT_REC * (int64_t)idx[3], fx, fy, r, tt);
        int32_t c = 0;
        for (int i = 0; i < m; ++i) {
            const double *p = rec + RESECT_REC * (int64_t)i;
            c += resect_inlier(r, tt, fx, fy, rho, p[0], p[1], p[2], p[3], p[4]) ? 1 : 0;
        }
        count[h] = valid ? c : -1;
    }
    return ransac_winner(H, [=](int32_t h) { return count[h]; }, [](int32_t h) { return h; });
}

static int32_t count_inliers(int32_t m, const double *rec, const double *R, const double *t, double fx, double fy, double rho)
{
    int32_t c = 0;
    for (int i = 0; i < m; ++i) {
        const double *p = rec + RESECT_REC * (int64_t)i;
        c += resect_inlier(R, t, fx, fy, rho, p[0], p[1], p[2], p[3], p[4]) ? 1 : 0;
    }
    return c;
}

void emul_orthonormalise(double *R) { resect_orthonormalise(R); }

// acc [RESECT_NSUM] = the sums of resect_accumulate at (P, q) over the inliers of (R, t), in one of three orders: 0 from the first
// correspondence to the last, 1 from the last to the first, 2 as 256 partial sums over every 256th correspondence (the strides of
// resect_refine_kernel's threads) added up in index order.  The device's tree is a fourth; what the order alone changes in a
// refined pose is measured between these.
static void sums(int32_t m, const double *rec, double fx, double fy, double rho, const double *R, const double *t, const double *P,
                 const double *q, int32_t order, double *acc)
{
    for (int k = 0; k < RESECT_NSUM; ++k) acc[k] = 0.0;
    const int lanes = order == 2 ? 256 : 1;
    for (int l = 0; l < lanes; ++l) {
        double part[RESECT_NSUM] = {};
        for (int k = l; k < m; k += lanes) {
            const double *p = rec + RESECT_REC * (int64_t)(order == 1 ? m - 1 - k : k);
            if (resect_inlier(R, t, fx, fy, rho, p[0], p[1], p[2], p[3], p[4])) resect_accumulate(P, q, fx, fy, p[0], p[1], p[2], p[3], p[4], part);
        }
        for (int k = 0; k < RESECT_NSUM; ++k) acc[k] = l == 0 ? part[k] : acc[k] + part[k];
    }
}

// The refinement rounds from (R, t) with `count` inliers, as resect_refine_kernel runs them; (R, t) in place, the new count
// returned; info [36] and rmse at the final pose over the final inliers.  order: see sums().
int32_t emul_refine(int32_t m, const double *rec, double fx, double fy, double rho, int32_t rounds, int32_t count, int32_t order, double *R,
                    double *t, double *info, double *rmse)
{
    double N36[36], acc[RESECT_NSUM];
    for (int round = 0; round < rounds && count > 0; ++round) {
        double P[9], q[3];
        for (int k = 0; k < 9; ++k) P[k] = R[k];
        for (int k = 0; k < 3; ++k) q[k] = t[k];
        bool ok = true;
        for (int step = 0; step < RESECT_GN_STEPS && ok; ++step) {
            sums(m, rec, fx, fy, rho, R, t, P, q, order, acc);
            ok = resect_step(acc, N36, P, q);
        }
        if (!ok) break;
        const int32_t cn = count_inliers(m, rec, P, q, fx, fy, rho);
        if (cn < count) break;
        count = cn;
        for (int k = 0; k < 9; ++k) R[k] = P[k];
        for (int k = 0; k < 3; ++k) t[k] = q[k];
    }
    sums(m, rec, fx, fy, rho, R, t, R, t, order, acc);
    int k = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) { info[6 * r + c] = acc[k]; info[6 * c + r] = acc[k]; ++k; }
    *rmse = count > 0 ? sqrt(acc[27] / (double)count) : 0.0;
    return count;
}

int32_t emul_status(int32_t m, int32_t min_inliers, int32_t count) { return ransac_status(m, RESECT_K, min_inliers, count); }

} // extern "C"
