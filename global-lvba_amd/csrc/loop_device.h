// loop_device.h -- loop-closure candidate search (lvba_loop_candidates): the scalar arithmetic of the rule.  Also compiles as
// plain C++ (tests/loop_check.cpp).  The including file is built without floating-point contraction: the radius gate and the
// orderings are discrete decisions on d2.
//   pos [n][3]: the frames' positions.  S = submap_size; submap w holds frames F_w = [w S, min((w + 1) S, n)).
//     d2(j, f) = ((dx dx + dy dy) + dz dz)                               fp64, rounded as written
//     (j, w) eligible iff |j - f| >= min_gap for every f in F_w, and min_f d2(j, f) <= radius radius
//     ref = the f of the smallest d2, the lowest f on a tie: the smallest (d2, f) pair in lexicographic order
//     per query the max_per_frame eligible submaps of the smallest (d2, w) pairs, written in the order of w
#pragma once
#include <math.h>
#include <stdint.h>
#include "visual_loss.h"

namespace lvba {

constexpr int LOOP_MAX_K = 32; // max_per_frame

struct LoopParams { // lvba_loop_opts on the device
    int32_t submap_size, min_gap, max_per_frame, query_stride;
    double radius2; // radius * radius
};

struct LoopBest { // a (d2, index) pair, ordered lexicographically
    double d2;
    int32_t idx;
};

LVBA_HD double loop_d2(const double *pos, int j, int f)
{
    const double dx = pos[3 * (int64_t)j] - pos[3 * (int64_t)f], dy = pos[3 * (int64_t)j + 1] - pos[3 * (int64_t)f + 1],
                 dz = pos[3 * (int64_t)j + 2] - pos[3 * (int64_t)f + 2];
    return (dx * dx + dy * dy) + dz * dz;
}

LVBA_HD bool loop_less(double d2a, int32_t ia, double d2b, int32_t ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// what a lane without a frame holds: loses against every real pair
LVBA_HD LoopBest loop_none()
{
    LoopBest b;
    b.d2 = INFINITY; b.idx = INT32_MAX;
    return b;
}

// |j - f| >= min_gap for every f of the (non-empty) run [f0, f1)
LVBA_HD bool loop_gap_ok(int j, int f0, int f1, int min_gap) { return min_gap <= 0 || j - (f1 - 1) >= min_gap || f0 - j >= min_gap; }

LVBA_HD bool loop_in_radius(double d2, double radius2) { return d2 <= radius2; }

// Keep the k best (d2, w) pairs seen so far in top[0 .. *n), ascending; ref[] rides along.
LVBA_HD void loop_keep(LoopBest *top, int32_t *ref, int *n, int k, double d2, int32_t w, int32_t f)
{
    int p = *n;
    if (p == k) {
        if (!loop_less(d2, w, top[k - 1].d2, top[k - 1].idx)) return;
        p = k - 1;
    } else {
        *n = p + 1;
    }
    while (p > 0 && loop_less(d2, w, top[p - 1].d2, top[p - 1].idx)) {
        top[p] = top[p - 1]; ref[p] = ref[p - 1];
        --p;
    }
    top[p].d2 = d2; top[p].idx = w; ref[p] = f;
}

// the kept pairs into the order of w (insertion sort; n <= LOOP_MAX_K)
LVBA_HD void loop_sort_by_submap(LoopBest *top, int32_t *ref, int n)
{
    for (int a = 1; a < n; ++a) {
        const LoopBest t = top[a];
        const int32_t r = ref[a];
        int p = a;
        while (p > 0 && top[p - 1].idx > t.idx) {
            top[p] = top[p - 1]; ref[p] = ref[p - 1];
            --p;
        }
        top[p] = t; ref[p] = r;
    }
}

#ifdef __HIPCC__
// One lane per query copies its count[q] staged entries (stage [nq][k]) to out[first[q] ..], up to `capacity` (the candidate
// searches: loop_candidates.hip, place.hip).
template <class Cand>
__global__ void loop_write_kernel(int nq, int k, const int64_t *__restrict__ count, const int64_t *__restrict__ first,
                                  const Cand *__restrict__ stage, int64_t capacity, Cand *__restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const int64_t c = count[q], d0 = first[q];
    for (int64_t a = 0; a < c && d0 + a < capacity; ++a) out[d0 + a] = stage[(int64_t)q * k + a];
}
#endif

} // namespace lvba
