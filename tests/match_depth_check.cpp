// match_depth_check.cpp -- the depth gate of csrc/match_device.h compiled for the host (tests/test_match_depth_host.py): the
// lifting and the predictions as their kernels call them, and the scan of one ordered pair walked the way match_scan_kernel walks
// it under the gate (see match_check.cpp) with the header's own update, merge and gate.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/match_device.h"

using namespace lvba;

extern "C" {

// world [n][3] of the keypoints of ONE image: uv [n][2] fp32 pixels, xy [n][2] undistorted, depth [h][w], (R, t) its pose
void emul_lift(int64_t n, const float *uv, const double *xy, const float *depth, int w, int h, const double *R, const double *t, double *world)
{
    for (int64_t i = 0; i < n; ++i) match_lift(depth, w, h, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1], R, t, world + 3 * i);
}

// pred [n][2]: the points world [n][3] in the image with pose (R, t)
void emul_predict(int64_t n, const double *intr, const double *R, const double *t, const double *world, double *pred)
{
    const TrkIntr cam{intr[0], intr[1], intr[2], intr[3], intr[4], intr[5], intr[6], intr[7]};
    for (int64_t i = 0; i < n; ++i) match_predict(cam, R, t, world + 3 * i, pred[2 * i], pred[2 * i + 1]);
}

// A [n_a][128], B [n_b][128]; uv_a, uv_b the pixels; pred_a [n_a][2] = a's keypoints in b, pred_b [n_b][2] = b's in a; best, s1, s2 [n_a]
void emul_scan_depth(int n_a, int n_b, const uint8_t *A, const uint8_t *B, const float *uv_a, const float *uv_b, const double *pred_a,
                     const double *pred_b, double rho2, int32_t *best, int32_t *s1, int32_t *s2)
{
    std::vector<int32_t> bias_a(n_a), bias_b(n_b);
    auto bias = [](const uint8_t *d) { int32_t s = 0; for (int k = 0; k < MATCH_DIM; ++k) s += (int32_t)d[k] - 128; return 128 * s; };
    for (int r = 0; r < n_a; ++r) bias_a[r] = bias(A + (int64_t)r * MATCH_DIM);
    for (int c = 0; c < n_b; ++c) bias_b[c] = bias(B + (int64_t)c * MATCH_DIM);
    for (int r = 0; r < n_a; ++r) {
        MatchTop top[32];
        for (int l = 0; l < 32; ++l) top[l] = match_top_none();
        const MatchReproj P{(double)uv_a[2 * r], (double)uv_a[2 * r + 1], pred_a[2 * r], pred_a[2 * r + 1]};
        for (int c0 = 0; c0 < n_b; c0 += 32)
            for (int l = 0; l < 32 && c0 + l < n_b; ++l) {
                const int c = c0 + l;
                int32_t acc = bias_b[c];
                for (int k = 0; k < MATCH_DIM; ++k)
                    acc += (int32_t)(int8_t)(A[(int64_t)r * MATCH_DIM + k] ^ 0x80) * (int32_t)(int8_t)(B[(int64_t)c * MATCH_DIM + k] ^ 0x80);
                const MatchReproj Q{(double)uv_b[2 * c], (double)uv_b[2 * c + 1], pred_b[2 * c], pred_b[2 * c + 1]};
                if (!match_depth_gate(P, Q, rho2)) acc = MATCH_NONE;
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

} // extern "C"
