// covis_check.cpp -- csrc/covis_device.h compiled for the host (tests/test_covis_host.py): the samples, the counts and the selection
// walked the way the kernels of covis.hip walk them, with the header's own functions.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/covis_device.h"

using namespace lvba;

namespace {
TrkIntr cam_of(const double *intr) { return TrkIntr{intr[0], intr[1], intr[2], intr[3], intr[4], intr[5], intr[6], intr[7]}; }
// rule: occlusion, both_ways, max_per_image, min_shared; bounds: min_overlap, occlusion_rel, occlusion_abs
CovisRule rule_of(const int32_t *rule, const double *bounds) { return CovisRule{rule[0], rule[1], rule[2], rule[3], bounds[0], bounds[1], bounds[2]}; }
} // namespace

extern "C" {

// world [M][G][3], ring [M][G]: as covis_lift_kernel, a cell per iteration
void emul_samples(int M, int w, int h, int grid_x, int grid_y, int radius, const float *depth, const double *Rcw, const double *tcw,
                  const double *intr, double *world, int32_t *ring)
{
    const TrkIntr cam = cam_of(intr);
    const int G = grid_x * grid_y;
    for (int64_t idx = 0; idx < (int64_t)M * G; ++idx) {
        const int m = (int)(idx / G), s = (int)(idx % G);
        ring[idx] = covis_sample(depth + (int64_t)m * w * h, w, h, cam, covis_centre(s % grid_x, grid_x, w), covis_centre(s / grid_x, grid_y, h),
                                 radius, Rcw + 9 * (int64_t)m, tcw + 3 * (int64_t)m, world + 3 * idx);
    }
}

// fate [M][M][G], n_points [M], counts [M][M]: as covis_count_kernel, a wavefront's (i, j) per iteration
void emul_counts(int M, int w, int h, int G, const float *depth, const double *Rcw, const double *tcw, const double *intr, const int32_t *rule,
                 const double *bounds, const double *world, int32_t *fate, int32_t *n_points, int32_t *counts)
{
    const TrkIntr cam = cam_of(intr);
    const CovisRule o = rule_of(rule, bounds);
    for (int j = 0; j < M; ++j)
        for (int i = 0; i < M; ++i) {
            int32_t total = 0;
            for (int s = 0; s < G; ++s) {
                const double *X = world + 3 * ((int64_t)i * G + s);
                const int f = i == j ? COVIS_NO_POINT : covis_fate(cam, depth + (int64_t)j * w * h, w, h, Rcw + 9 * (int64_t)j, tcw + 3 * (int64_t)j, X, o);
                fate[((int64_t)i * M + j) * G + s] = f;
                const bool hit = i == j ? X[0] == X[0] : covis_seen(cam, depth + (int64_t)j * w * h, w, h, Rcw + 9 * (int64_t)j, tcw + 3 * (int64_t)j, X, o);
                total += hit ? 1 : 0;
            }
            if (i == j) n_points[i] = total;
            counts[(int64_t)i * M + j] = i == j ? 0 : total;
        }
}

// pairs [M (M - 1) / 2][2], score, shared [..][2]; returns the number kept: as covis_select_kernel (K rounds, each behind the last)
// and covis_write_kernel
int64_t emul_select(int M, const int32_t *rule, const double *bounds, const int32_t *n_points, const int32_t *counts, int32_t *pairs,
                    double *score, int32_t *shared)
{
    const CovisRule o = rule_of(rule, bounds);
    const int K = o.max_per_image;
    auto pair_of = [&](int i, int j) { return covis_pair(counts[(int64_t)i * M + j], counts[(int64_t)j * M + i], n_points[i], n_points[j], o); };
    std::vector<CovisRank> kth((size_t)M, covis_rank_last());
    for (int i = 0; i < M && K > 0; ++i) {
        CovisRank prev = covis_rank_first();
        for (int k = 0; k < K; ++k) {
            CovisRank best = covis_rank_last();
            for (int p = 0; p < M; ++p) {
                if (p == i) continue;
                const CovisPair pr = pair_of(i, p);
                const CovisRank c{pr.score, p};
                if (pr.eligible && covis_rank_before(prev, c) && covis_rank_before(c, best)) best = c;
            }
            prev = best;
            if (best.partner == INT32_MAX) break;
        }
        kth[(size_t)i] = prev;
    }
    int64_t n = 0;
    for (int i = 0; i < M; ++i)
        for (int j = i + 1; j < M; ++j) {
            const CovisPair pr = pair_of(i, j);
            if (!pr.eligible) continue;
            if (K > 0 && !covis_within_cap(pr.score, j, kth[(size_t)i]) && !covis_within_cap(pr.score, i, kth[(size_t)j])) continue;
            pairs[2 * n] = i; pairs[2 * n + 1] = j;
            score[n] = pr.score;
            shared[2 * n] = counts[(int64_t)i * M + j]; shared[2 * n + 1] = counts[(int64_t)j * M + i];
            ++n;
        }
    return n;
}

} // extern "C"
