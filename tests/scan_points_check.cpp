// scan_points_check.cpp -- csrc/scan_points.h compiled for the host (tests/test_ordering.py): the leaf key, its squared distance
// and the key packing against the expressions of down_sampling_voxel2 written out literally, at the edges of the rule;
// pose_apply against the written-out rows.  Built with -ffp-contract=off like the files that call leaf_key_of.  (The frame
// search against a linear scan, in both offset dialects: tests/segments_check.cpp, with the search it forwards to.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "../global-lvba_amd/csrc/scan_points.h"

using namespace lvba;

static int fails = 0;
#define CHECK(cond, ...)                                                                                                    \
    do {                                                                                                                    \
        if (!(cond)) {                                                                                                      \
            if (++fails <= 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                   \
    } while (0)

// one point against the literal rule: tools.hpp:318-341, and the range clause of the packing
static void check_leaf(const float q[3], double leaf)
{
    bool want_ok = true;
    int64_t want_k[3];
    double want_d2 = 0.0;
    for (int j = 0; j < 3; ++j) {
        float loc = (float)((double)q[j] / leaf);
        if (loc < 0) loc -= 1.0f;
        if (!(std::fabs(loc) < 1048576.0f)) { want_ok = false; break; } // also NaN
        want_k[j] = (int64_t)loc;
    }
    int64_t k[3] = {7, 7, 7};
    double d2 = -1.0;
    const bool ok = leaf_key_of(q, leaf, k, d2);
    CHECK(ok == want_ok, "q = (%a, %a, %a) leaf %g: returned %d, literal %d", q[0], q[1], q[2], leaf, (int)ok, (int)want_ok);
    if (!ok || !want_ok) return;
    for (int j = 0; j < 3; ++j) {
        const double c = ((double)want_k[j] + 0.5) * leaf, d = (double)q[j] - c;
        want_d2 = want_d2 + d * d;
        CHECK(k[j] == want_k[j], "q[%d] = %a leaf %g: key %lld, literal %lld", j, q[j], leaf, (long long)k[j], (long long)want_k[j]);
    }
    CHECK(d2 == want_d2, "q = (%a, %a, %a) leaf %g: d2 %a, literal %a", q[0], q[1], q[2], leaf, d2, want_d2);
    const uint64_t key = pack_key(k);
    const uint64_t want_key = ((uint64_t)(want_k[0] + 1048576) << 42) | ((uint64_t)(want_k[1] + 1048576) << 21) | (uint64_t)(want_k[2] + 1048576);
    CHECK(key == want_key, "pack %llx, literal %llx", (unsigned long long)key, (unsigned long long)want_key);
    CHECK((int64_t)(key >> 42) == k[0] + KEY_BIAS && (int64_t)((key >> 21) & 0x1fffff) == k[1] + KEY_BIAS &&
              (int64_t)(key & 0x1fffff) == k[2] + KEY_BIAS,
          "unpacking %llx does not give back k + KEY_BIAS", (unsigned long long)key);
}

int main()
{
    static_assert(KEY_BIAS == 1 << 20, "3 x 21 bits");
    const float eps = 1.0f / 8388608.0f; // 2^-23
    for (const double leaf : {0.01, 0.1, 0.5, 1.0}) {
        const float l = (float)leaf;
        const float top = (float)(1048575.0 * leaf), out = (float)(1048576.0 * leaf);
        const float v[] = {0.0f, -0.0f, l, -l, l * (1.0f + eps), l * (1.0f - eps), -l * (1.0f + eps), -l * (1.0f - eps),
                           top, -top, out, -out, std::numeric_limits<float>::quiet_NaN(), 0.37f * l};
        const int nv = (int)(sizeof(v) / sizeof(v[0]));
        for (int a = 0; a < nv; ++a)
            for (int b = 0; b < nv; ++b)
                for (int c = 0; c < nv; ++c) {
                    const float q[3] = {v[a], v[b], v[c]};
                    check_leaf(q, leaf);
                }
        // the edges of the packable range on their own: (2^20 - 1) leaves is the last key, 2^20 leaves and NaN are refused.
        // -(2^20 - 1) leaves is refused as well: "minus one for negatives" takes it to -2^20, and the rule asks |loc| < 2^20
        // after that step (the literal above; so did every copy of the rule before they became this one).
        int64_t k[3];
        double d2;
        const float in[3] = {top, 0.0f, 0.0f}, neg[3] = {0.0f, -top, 0.0f}, hi[3] = {0.0f, 0.0f, out}, lo[3] = {-out, 0.0f, 0.0f},
                    nan[3] = {0.0f, std::numeric_limits<float>::quiet_NaN(), 0.0f};
        CHECK(leaf_key_of(in, leaf, k, d2) && k[0] == 1048575 && k[1] == 0 && k[2] == 0, "leaf %g: +(2^20 - 1) leaves", leaf);
        CHECK(!leaf_key_of(neg, leaf, k, d2), "leaf %g: -(2^20 - 1) leaves", leaf);
        CHECK(!leaf_key_of(hi, leaf, k, d2), "leaf %g: +2^20 leaves", leaf);
        CHECK(!leaf_key_of(lo, leaf, k, d2), "leaf %g: -2^20 leaves", leaf);
        CHECK(!leaf_key_of(nan, leaf, k, d2), "leaf %g: NaN", leaf);
    }

    const double T[12] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6, 1.25, -3.5, 0.0625};
    const float p[][3] = {{1.5f, -2.25f, 0.3f}, {-17.1f, 4.4f, 19.9f}, {0.0f, 0.0f, 0.0f}};
    for (const auto &x : p) {
        const double p0 = x[0], p1 = x[1], p2 = x[2];
        const double want[3] = {T[0] * p0 + T[1] * p1 + T[2] * p2 + T[9], T[3] * p0 + T[4] * p1 + T[5] * p2 + T[10],
                                T[6] * p0 + T[7] * p1 + T[8] * p2 + T[11]};
        double w[3];
        float wf[3];
        pose_apply(T, x[0], x[1], x[2], w);
        pose_apply_f32(T, x[0], x[1], x[2], wf);
        for (int j = 0; j < 3; ++j) CHECK(w[j] == want[j] && wf[j] == (float)want[j], "pose_apply row %d", j);
    }

    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("scan points ok\n");
    return 0;
}
