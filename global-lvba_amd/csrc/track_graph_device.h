// track_graph_device.h -- scalar pieces of the device track builder (track_graph.hip; the rule is in include/lvba_hip.h, DESIGN.md
// §10j): where a match's two half-edges go, the label step of the connected components, the run heads and the two size checks of
// the member pass, and the queue bookkeeping of the BFS.  Integer-only.  Host/device-neutral, like match_device.h and
// covis_device.h: tests/track_graph_check.cpp walks the same functions on the CPU the way the kernels walk them.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "segments.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LVBA_TG_FN __host__ __device__ __forceinline__
#else
#define LVBA_TG_FN inline
#endif

namespace lvba {

constexpr int64_t TG_MAX_NODES = (int64_t)1 << 31;   // kp_off[M] below this: node ids and the "no node" key fit in 32 bits
constexpr int64_t TG_MAX_MATCHES = (int64_t)1 << 30; // match_off[n_pairs] below this: half-edge ids fit in 32 bits
constexpr int TG_MAX_ROUNDS = 64;                    // label rounds; the number of trees at least halves per round
constexpr int TG_JUMP_STEPS = 32;                    // pointer-jumping steps of one thread in one round

// TG_BFS_LANES lanes of a wavefront walk one component: 8, eight components per wavefront.  A compile-time choice; DESIGN.md §10j
// has what 64 (a wavefront per component) gave.
#ifndef LVBA_TG_BFS_LANES
#define LVBA_TG_BFS_LANES 8
#endif
constexpr int TG_BFS_LANES = LVBA_TG_BFS_LANES;
static_assert(TG_BFS_LANES == 64 || TG_BFS_LANES == 32 || TG_BFS_LANES == 16 || TG_BFS_LANES == 8, "a power of two that divides 64");

enum TgError : uint32_t { TG_OK = 0, TG_ERR_OVERRUN = 1, TG_ERR_SHORT = 2 };

// the last index i in [0, n] with off[i] <= x, segment_of over the n + 1 entries of off: a node's image (n = M - 1), a row's pair
LVBA_TG_FN int64_t tg_owner(const int64_t *__restrict__ off, int64_t n, int64_t x) { return segment_of(off, n + 1, x); }

// Host: the pairs ranked by a stable sort on (lo, hi); first_seq [n_pairs] = the sequence number of each pair's first match.
inline void tg_rank_pairs(int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, std::vector<int64_t> &first_seq)
{
    std::vector<int64_t> rank((size_t)n_pairs);
    std::iota(rank.begin(), rank.end(), (int64_t)0);
    std::stable_sort(rank.begin(), rank.end(), [&](int64_t x, int64_t y) {
        const int32_t xl = std::min(pairs[2 * x], pairs[2 * x + 1]), xh = std::max(pairs[2 * x], pairs[2 * x + 1]);
        const int32_t yl = std::min(pairs[2 * y], pairs[2 * y + 1]), yh = std::max(pairs[2 * y], pairs[2 * y + 1]);
        return xl != yl ? xl < yl : xh < yh;
    });
    first_seq.assign((size_t)n_pairs, 0);
    int64_t seq = 0;
    for (int64_t p : rank) { first_seq[(size_t)p] = seq; seq += match_off[p + 1] - match_off[p]; }
}

// Match row `row` of the caller's arrays -> its two half-edges.  pairs [n_pairs][2], match_off [n_pairs + 1], first_seq [n_pairs]:
// the sequence number of each pair's first match in rank order.  Writes (src, dst) at 2 e and 2 e + 1 of the sequence order; a
// skipped match gets the key n_nodes_total, which sorts behind every node.  Returns e.
LVBA_TG_FN int64_t tg_half_edges(int64_t row, int64_t n_pairs, const int32_t *__restrict__ pairs, const int64_t *__restrict__ match_off,
                                 const int64_t *__restrict__ first_seq, const int32_t *__restrict__ matches, const int64_t *__restrict__ kp_off,
                                 uint32_t no_node, uint32_t *__restrict__ src, uint32_t *__restrict__ dst)
{
    const int64_t p = tg_owner(match_off, n_pairs - 1, row);
    const int64_t e = first_seq[p] + (row - match_off[p]);
    int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    int32_t r = matches[2 * row], c = matches[2 * row + 1];
    if (a > b) { const int32_t t = a; a = b; b = t; const int32_t u = r; r = c; c = u; } // read as (lo, hi)
    const int64_t na = kp_off[a + 1] - kp_off[a], nb = kp_off[b + 1] - kp_off[b];
    const bool ok = r >= 0 && c >= 0 && r < na && c < nb;
    const uint32_t u = ok ? (uint32_t)(kp_off[a] + r) : no_node, v = ok ? (uint32_t)(kp_off[b] + c) : no_node;
    src[2 * e] = u; dst[2 * e] = v;
    src[2 * e + 1] = v; dst[2 * e + 1] = u;
    return e;
}

// the first position of sorted key [n] that holds a key >= v: the start of node v's neighbours
LVBA_TG_FN uint32_t tg_lower_bound(const uint32_t *__restrict__ key, uint32_t n, uint32_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define LVBA_TG_MIN(ptr, val) atomicMin((ptr), (val))
#else
LVBA_TG_FN uint32_t tg_host_min(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v < old) *p = v; return old; }
#define LVBA_TG_MIN(ptr, val) tg_host_min((ptr), (val))
#endif

// Label step over one half-edge (u, v): labels only ever decrease, every label names a node of the same component that is not
// larger than the node itself.  The smaller of the two ends' labels is offered to the other end and to the other end's label
// (hooking a tree's root under a smaller one).  Returns whether anything was lowered.  The only fixed point of the rounds is
// "every label is its component's smallest node", whatever the order in which the edges are taken.
LVBA_TG_FN bool tg_hook(uint32_t *label, uint32_t u, uint32_t v)
{
    const uint32_t lu = label[u], lv = label[v];
    if (lu >= lv) return false; // the twin half-edge (v, u) handles lu > lv
    const bool a = LVBA_TG_MIN(&label[lv], lu) > lu;
    const bool b = LVBA_TG_MIN(&label[v], lu) > lu;
    return a || b;
}

// Pointer jumping of node v, at most TG_JUMP_STEPS steps: label[v] <- label[label[v]].  Only v's own label is written.
LVBA_TG_FN bool tg_jump(uint32_t *label, uint32_t v)
{
    uint32_t l = label[v];
    bool changed = false;
    for (int k = 0; k < TG_JUMP_STEPS; ++k) {
        const uint32_t ll = label[l];
        if (ll == l) break;
        l = ll; changed = true;
    }
    if (changed) label[v] = l;
    return changed;
}

// Member pass over position i of the nodes sorted (stably) by label: head of a run, and whether the image changes here.
LVBA_TG_FN bool tg_run_head(const uint32_t *__restrict__ lab, int64_t i) { return i == 0 || lab[i] != lab[i - 1]; }
LVBA_TG_FN bool tg_image_change(const uint32_t *__restrict__ lab, const int32_t *__restrict__ img, int64_t i)
{
    return tg_run_head(lab, i) || img[i] != img[i - 1];
}
// the two size checks of src/lvba_system.cpp:983-1014
LVBA_TG_FN bool tg_qualifies(uint32_t size, uint32_t images, int32_t obser_thr)
{
    return size >= (uint32_t)obser_thr && images >= (uint32_t)obser_thr;
}

// BFS bookkeeping: how many of `n_new` nodes may be appended to a queue that holds `tail` of `size`.  An append beyond the
// component's size never happens: the walk ends with TG_ERR_OVERRUN instead.
LVBA_TG_FN bool tg_append_fits(uint32_t tail, uint32_t n_new, uint32_t size) { return n_new <= size - tail; }

} // namespace lvba
