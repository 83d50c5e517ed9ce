// ransac_device.h -- what the batched RANSAC stages have in common, as far as it is plain arithmetic (verify.hip, resect.hip;
// DESIGN.md §10k "The skeleton"): the counter-based generator, the sampler of K distinct positions, the rank of a hypothesis, the
// winner over a sequence of them, the status of a task, and the list of (task, block of hypotheses) tiles that the hypothesis
// kernel's grid is.  Host/device-neutral and integer-only, no HIP calls: the host checks compile it with g++ as it stands
// (tests/verify_check.cpp, tests/resect_check.cpp, tests/ransac_check.cpp).  The kernels and launches built on it are in
// ransac_batch.h; the model, its solver, its inlier test and its refit are the stage's own (verify_device.h, resect_device.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "tracks_device.h"

namespace lvba {

// lvba_verify_* and lvba_resect_* report these values (include/lvba_hip.h)
enum RansacStatus : int { RANSAC_OK = 0, RANSAC_TOO_FEW_MATCHES = 1, RANSAC_NO_MODEL = 2, RANSAC_TOO_FEW_INLIERS = 3 };
constexpr uint64_t RANSAC_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int64_t RANSAC_MAX_BLOCKS = INT32_MAX / 2;   // hypothesis blocks in one call: the block records are indexed in 32 bits

// ---- the generator: a function of (seed, lo, hi, h, draw) alone -- not of the task's place in the call, the grid or the lane ----
LVBA_TRK_FN uint64_t ransac_mix(uint64_t z)        // splitmix64's finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
LVBA_TRK_FN uint64_t ransac_key(uint64_t seed, int32_t lo, int32_t hi, int32_t h)
{
    uint64_t k = ransac_mix(seed + RANSAC_GOLDEN);
    k = ransac_mix(k ^ (((uint64_t)(uint32_t)lo << 32) | (uint64_t)(uint32_t)hi));
    return ransac_mix(k + RANSAC_GOLDEN * ((uint64_t)(uint32_t)h + 1));
}
LVBA_TRK_FN uint64_t ransac_draw(uint64_t key, int j) { return ransac_mix(key + RANSAC_GOLDEN * ((uint64_t)j + 1)); }
LVBA_TRK_FN uint32_t ransac_below(uint64_t r, uint32_t n)   // the high half of r n: r mapped onto [0, n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul64hi(r, (uint64_t)n);
#else
    return (uint32_t)(((unsigned __int128)r * n) >> 64);
#endif
}
// K distinct indices of [0, m), m >= K, in draw order: draw j is taken from [0, m - j) and stepped past the indices already
// chosen, which `sorted` keeps in ascending order (a partial Fisher-Yates shuffle without its array).
template <int K>
LVBA_TRK_FN void ransac_sample(uint64_t key, int32_t m, int32_t *idx)
{
    int32_t sorted[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int32_t v = (int32_t)ransac_below(ransac_draw(key, j), (uint32_t)(m - j));
#pragma unroll
        for (int i = 0; i < j; ++i) v += v >= sorted[i] ? 1 : 0;
        idx[j] = v;
        sorted[j] = v;
#pragma unroll
        for (int i = j; i > 0; --i)
            if (sorted[i - 1] > sorted[i]) { const int32_t s = sorted[i - 1]; sorted[i - 1] = sorted[i]; sorted[i] = s; }
    }
}

// ---- the choice -------------------------------------------------------------------------------------------------------------------
// The highest count wins, the lowest h among equals; an invalid hypothesis counts -1.  Integers only: no reduction order matters.
LVBA_TRK_FN int64_t ransac_rank(int32_t count, int32_t h) { return ((int64_t)(count + 1) << 32) | (int64_t)(uint32_t)(INT32_MAX - h); }
// The winner among n candidates, candidate k being hypothesis h(k) with count(k): the k of the highest rank; -1 when there is no
// candidate or the best of them is invalid.
template <class Count, class Hyp>
LVBA_TRK_FN int32_t ransac_winner(int32_t n, const Count &count, const Hyp &h)
{
    int32_t win = -1;
    int64_t top = -1;
    for (int32_t k = 0; k < n; ++k) {
        const int64_t r = ransac_rank(count(k), h(k));
        if (r > top) { top = r; win = k; }
    }
    return win >= 0 && count(win) >= 0 ? win : -1;
}
// m elements, samples of k, `count` inliers of the final model (-1: every hypothesis invalid)
LVBA_TRK_FN int ransac_status(int32_t m, int32_t k, int32_t min_inliers, int32_t count)
{
    if (m < (k > min_inliers ? k : min_inliers)) return RANSAC_TOO_FEW_MATCHES;
    if (count < 0) return RANSAC_NO_MODEL;
    return count < min_inliers ? RANSAC_TOO_FEW_INLIERS : RANSAC_OK;
}

// ---- the tile list ----------------------------------------------------------------------------------------------------------------
// A task's elements in the call's arrays and its block records; every task struct holds one as its member `span`.
struct RansacSpan {
    int64_t off;                    // first element (match, correspondence) of the task
    int32_t m;                      // elements
    int32_t blk0, n_blk;            // block records [blk0, blk0 + n_blk): one per tile of the task
};
struct alignas(8) RansacTile { int32_t task, h0; };   // hypotheses [h0, h0 + hb) of the task
// The grid of the hypothesis kernel: every task with span.m >= need gets ceil(H / hb) blocks, in task order; the others none, and
// their blk0 is where their blocks would have started.  Sets blk0 / n_blk, fills `tiles` (null: the count alone) -- block k of
// task p is tile blk0 + k = (p, k hb) -- and returns the number of blocks; or -1, nothing built and the tasks untouched, when
// there would be more than RANSAC_MAX_BLOCKS: counted in 64 bits first, so that no H >= 1 overflows anything.
template <class Task>
inline int64_t ransac_plan(Task *tasks, size_t n_tasks, int32_t H, int32_t hb, int32_t need, std::vector<RansacTile> *tiles)
{
    const int64_t per = ((int64_t)H + hb - 1) / hb;
    int64_t eligible = 0, n = 0;
    for (size_t p = 0; p < n_tasks; ++p) eligible += tasks[p].span.m >= need ? 1 : 0;
    if (eligible * per > RANSAC_MAX_BLOCKS) return -1;   // both factors are below 2^31
    if (tiles) { tiles->clear(); tiles->reserve((size_t)(eligible * per)); }
    for (size_t p = 0; p < n_tasks; ++p) {
        RansacSpan &sp = tasks[p].span;
        sp.blk0 = (int32_t)n;
        sp.n_blk = sp.m >= need ? (int32_t)per : 0;
        n += sp.n_blk;
        for (int64_t k = 0; tiles && k < sp.n_blk; ++k) tiles->push_back(RansacTile{(int32_t)p, (int32_t)(k * hb)});
    }
    return n;
}

} // namespace lvba
