// match_check.cpp -- csrc/match_device.h compiled for the host (tests/test_match_host.py): the scan of one ordered pair walked the
// way match_scan_kernel walks it -- signed bytes with the column bias as the accumulator's start, 32 column lanes per row that
// meet their columns in ascending order, the xor butterfly at the end, the row constant last -- with the header's own update,
// merge, gate and decision.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/match_device.h"

using namespace lvba;

extern "C" {

void emul_essential(const double *Rlo, const double *tlo, const double *Rhi, const double *thi, double *E)
{
    match_essential(Rlo, tlo, Rhi, thi, E);
}

// xy [n][2], NaN where the undistortion fails
void emul_undistort(int64_t n, const float *uv, const double *intr, double *xy)
{
    const TrkIntr cam{intr[0], intr[1], intr[2], intr[3], intr[4], intr[5], intr[6], intr[7]};
    for (int64_t i = 0; i < n; ++i) {
        double x, y;
        if (!trk_undistort(cam, (double)uv[2 * i], (double)uv[2 * i + 1], x, y)) x = y = NAN;
        xy[2 * i] = x; xy[2 * i + 1] = y;
    }
}

// A [n_a][128], B [n_b][128]; guided: E (lo -> hi), xy_a, xy_b, tau2, rows_lo as the kernel's task; best, s1, s2 [n_a]
void emul_scan(int n_a, int n_b, const uint8_t *A, const uint8_t *B, int guided, int rows_lo, const double *E, const double *xy_a,
               const double *xy_b, double tau2, int32_t *best, int32_t *s1, int32_t *s2)
{
    std::vector<int32_t> bias_a(n_a), bias_b(n_b);
    auto bias = [](const uint8_t *d) { int32_t s = 0; for (int k = 0; k < MATCH_DIM; ++k) s += (int32_t)d[k] - 128; return 128 * s; };
    for (int r = 0; r < n_a; ++r) bias_a[r] = bias(A + (int64_t)r * MATCH_DIM);
    for (int c = 0; c < n_b; ++c) bias_b[c] = bias(B + (int64_t)c * MATCH_DIM);
    for (int r = 0; r < n_a; ++r) {
        MatchTop top[32];
        for (int l = 0; l < 32; ++l) top[l] = match_top_none();
        MatchLine P{};
        if (guided) {
            const double x = xy_a[2 * r], y = xy_a[2 * r + 1];
            if (rows_lo) P = match_line_lo(E, x, y);
            else { P.l0 = x; P.l1 = y; P.l2 = 0.0; P.n = match_norm_hi(E, x, y); }
        }
        for (int c0 = 0; c0 < n_b; c0 += 32)
            for (int l = 0; l < 32 && c0 + l < n_b; ++l) {
                const int c = c0 + l;
                int32_t acc = bias_b[c];
                for (int k = 0; k < MATCH_DIM; ++k)
                    acc += (int32_t)(int8_t)(A[(int64_t)r * MATCH_DIM + k] ^ 0x80) * (int32_t)(int8_t)(B[(int64_t)c * MATCH_DIM + k] ^ 0x80);
                if (guided) {
                    const double cx = xy_b[2 * c], cy = xy_b[2 * c + 1];
                    const bool pass = rows_lo ? match_gate(P, cx, cy, match_norm_hi(E, cx, cy), tau2)
                                              : match_gate(match_line_lo(E, cx, cy), P.l0, P.l1, P.n, tau2);
                    if (!pass) acc = MATCH_NONE;
                }
                match_top_update(top[l], acc, c);
            }
        for (int m = 1; m < 32; m <<= 1) {
            MatchTop next[32];
            for (int l = 0; l < 32; ++l) next[l] = match_top_merge(top[l], top[l ^ m]);
            for (int l = 0; l < 32; ++l) top[l] = next[l];
        }
        const int32_t rc = bias_a[r] + MATCH_BIAS_CONST;
        best[r] = top[0].best;
        s1[r] = top[0].best >= 0 ? top[0].s1 + rc : 0;
        s2[r] = top[0].s2 != MATCH_NONE ? top[0].s2 + rc : 0;
    }
}

int emul_accept(int32_t best, int32_t s1, int32_t s2, double max_distance, double max_ratio)
{
    return match_accept(best, s1, s2, max_distance, max_ratio) ? 1 : 0;
}

} // extern "C"
