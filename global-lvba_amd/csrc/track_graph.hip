// track_graph.hip -- feature tracks on the device: the key point match graph, its connected components, the two size checks and
// the BFS order of every component that lvba_fuse_tracks consumes (lvba_trackgraph_*; the rule is in include/lvba_hip.h, its
// scalar pieces in track_graph_device.h).
//
// Device design:
//   trackgraph_edge_kernel    a thread per match row: its pair by a search in match_off, its two half-edges at 2 e and 2 e + 1 of the
//                             sequence order (the host ranks the n_pairs pairs; a skipped match gets the key "no node").
//   rocprim radix sort        stable, by src over the bits that vary: the CSR adjacency in the rule's order.
//   trackgraph_offsets_kernel a thread per node: where its neighbours start (a search in the sorted keys).
//   trackgraph_hook_kernel,   label rounds: a thread per half-edge offers the smaller end's label to the other end and to that
//   trackgraph_jump_kernel    end's label (atomicMin), then a thread per node jumps its pointer; until a round changes nothing.
//                             THE ONLY ATOMICS OF THIS FILE.  The fixed point is unique -- every label is its component's smallest
//                             node --, so the labels are the same bytes under any schedule; only the number of rounds may differ.
//   trackgraph_nodes_kernel   flag / scan / write: the nodes with an edge, ascending; a stable radix sort by label then gives the
//                             members of all components, each a contiguous run in scan order, the runs by smallest member.
//   trackgraph_runs_kernel .. run heads and image changes along the sorted nodes, two scans, sizes and distinct images per run, the
//   trackgraph_table_kernel   two size checks, a scan of the flags, the compacted component table (first, size, images).
//   trackgraph_members_kernel lvba_trackgraph_components: a thread per observation of the qualifying components.
//   trackgraph_bfs_kernel     lvba_trackgraph_orders: TG_BFS_LANES lanes per requested component; the component's segment of the
//                             output is the queue.  Visited marks are a resident uint32 stamp per node against a per-call epoch.
//                             For a popped node the lanes take its neighbours a batch at a time, drop the stamped ones, resolve
//                             equal unseen neighbours to the lowest lane, and append in lane order.  Then the same lanes turn the
//                             queue into (image, key point, uv).
// Every device loop is bounded by a size: the rounds by TG_MAX_ROUNDS, a jump by TG_JUMP_STEPS, the BFS by head < tail <= size.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "segments.h"
#include "image_set.h"
#include "track_graph_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

struct lvba_trackgraph_s {
    ImageSet kp;                         // the images' offsets on the device (kp.off.back() nodes), their pixels where given
    int32_t obser_thr = 0;
    bool has_uv = false;
    uint32_t epoch = 0;
    lvba_trackgraph_info info{};
    std::vector<uint32_t> comp_size, comp_images; // [n_components]
    uint32_t *d_adj_off = nullptr;       // [N + 1]
    uint32_t *d_adj = nullptr;           // [2 n_edges (+ 2 n_skipped behind them)]
    uint32_t *d_members = nullptr;       // [n_nodes] the nodes with an edge, by (label, node)
    uint32_t *d_stamp = nullptr;         // [N]
    uint32_t *d_comp_first = nullptr;    // [n_components] first member in d_members
    uint32_t *d_comp_size = nullptr;     // [n_components]
    uint32_t *d_comp_obs = nullptr;      // [n_components + 1] first observation of lvba_trackgraph_components
};

namespace {

constexpr int TG_BLOCK = 256;

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_edge_kernel(int64_t n_matches, int64_t n_pairs, const int32_t *__restrict__ pairs,
                                                                   const int64_t *__restrict__ match_off, const int64_t *__restrict__ first_seq,
                                                                   const int32_t *__restrict__ matches, const int64_t *__restrict__ kp_off,
                                                                   uint32_t no_node, uint32_t *__restrict__ src, uint32_t *__restrict__ dst)
{
    const int64_t row = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (row >= n_matches) return;
    tg_half_edges(row, n_pairs, pairs, match_off, first_seq, matches, kp_off, no_node, src, dst);
}

// adj_off [N + 1]
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_offsets_kernel(int64_t N, const uint32_t *__restrict__ key, uint32_t n_half,
                                                                      uint32_t *__restrict__ adj_off)
{
    const int64_t v = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (v > N) return;
    adj_off[v] = tg_lower_bound(key, n_half, (uint32_t)v);
}

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_iota_kernel(int64_t N, uint32_t *__restrict__ label)
{
    const int64_t v = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (v < N) label[v] = (uint32_t)v;
}

// n_half: the half-edges of the matches that were not skipped (the sorted prefix)
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_hook_kernel(uint32_t n_half, const uint32_t *__restrict__ key, const uint32_t *__restrict__ adj,
                                                                   uint32_t *label, uint32_t *changed)
{
    const int64_t i = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i >= n_half) return;
    if (tg_hook(label, key[i], adj[i])) *changed = 1u;
}

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_jump_kernel(int64_t N, uint32_t *label, uint32_t *changed)
{
    const int64_t v = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (v >= N) return;
    if (tg_jump(label, (uint32_t)v)) *changed = 1u;
}

// flag [N + 1]: node v has an edge (the last is 0)
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_degree_kernel(int64_t N, const uint32_t *__restrict__ adj_off, uint32_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (v > N) return;
    flag[v] = v < N && adj_off[v + 1] > adj_off[v] ? 1u : 0u;
}

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_nodes_kernel(int64_t N, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                                    const uint32_t *__restrict__ label, uint32_t *__restrict__ node,
                                                                    uint32_t *__restrict__ node_label)
{
    const int64_t v = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (v >= N || !flag[v]) return;
    node[excl[v]] = (uint32_t)v;
    node_label[excl[v]] = label[v];
}

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_image_kernel(int64_t n_nodes, const uint32_t *__restrict__ members, const int64_t *__restrict__ kp_off,
                                                                    int32_t M, int32_t *__restrict__ img)
{
    const int64_t i = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i < n_nodes) img[i] = (int32_t)tg_owner(kp_off, M - 1, (int64_t)members[i]);
}

// head, change [n_nodes + 1] (the last of each is 0)
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_runs_kernel(int64_t n_nodes, const uint32_t *__restrict__ lab, const int32_t *__restrict__ img,
                                                                   uint32_t *__restrict__ head, uint32_t *__restrict__ change)
{
    const int64_t i = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i > n_nodes) return;
    head[i] = i < n_nodes && tg_run_head(lab, i) ? 1u : 0u;
    change[i] = i < n_nodes && tg_image_change(lab, img, i) ? 1u : 0u;
}

// run_first [n_all + 1]: the position of each run's head, and n_nodes behind the last
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_heads_kernel(int64_t n_nodes, const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_of,
                                                                    uint32_t *__restrict__ run_first)
{
    const int64_t i = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i > n_nodes) return;
    if (i == n_nodes || head[i]) run_first[run_of[i]] = (uint32_t)i;
}

// keep [n_all + 1] (the last is 0), kept_size [n_all + 1]: the size of a run that passes the two checks, else 0
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_check_kernel(int64_t n_all, const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ change_x,
                                                                    int32_t obser_thr, uint32_t *__restrict__ keep, uint32_t *__restrict__ kept_size)
{
    const int64_t r = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (r > n_all) return;
    bool ok = false;
    uint32_t size = 0;
    if (r < n_all) {
        const uint32_t a = run_first[r], b = run_first[r + 1];
        size = b - a;
        ok = tg_qualifies(size, change_x[b] - change_x[a], obser_thr);
    }
    keep[r] = ok ? 1u : 0u;
    kept_size[r] = ok ? size : 0u;
}

// the compacted table; comp_obs [n_components + 1] gets its last entry from the run behind the last
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_table_kernel(int64_t n_all, const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ change_x,
                                                                    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ comp_of,
                                                                    const uint32_t *__restrict__ obs_x, uint32_t *__restrict__ comp_first,
                                                                    uint32_t *__restrict__ comp_size, uint32_t *__restrict__ comp_images,
                                                                    uint32_t *__restrict__ comp_obs)
{
    const int64_t r = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (r > n_all) return;
    if (r == n_all) { comp_obs[comp_of[r]] = obs_x[r]; return; }
    if (!keep[r]) return;
    const uint32_t c = comp_of[r], a = run_first[r], b = run_first[r + 1];
    comp_first[c] = a; comp_size[c] = b - a; comp_images[c] = change_x[b] - change_x[a]; comp_obs[c] = obs_x[r];
}

__global__ __launch_bounds__(TG_BLOCK) void trackgraph_members_kernel(int64_t n_obs, uint32_t n_comp, const uint32_t *__restrict__ comp_obs,
                                                                      const uint32_t *__restrict__ comp_first, const uint32_t *__restrict__ members,
                                                                      const int64_t *__restrict__ kp_off, int32_t M, int32_t *__restrict__ mem_img,
                                                                      int32_t *__restrict__ mem_kp)
{
    const int64_t j = (int64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (j >= n_obs) return;
    const uint32_t lo = segment_of(comp_obs, n_comp, (uint32_t)j);
    const uint32_t node = members[comp_first[lo] + ((uint32_t)j - comp_obs[lo])];
    const int64_t i = tg_owner(kp_off, M - 1, (int64_t)node);
    mem_img[j] = (int32_t)i;
    mem_kp[j] = (int32_t)((int64_t)node - kp_off[i]);
}

__device__ __forceinline__ uint32_t load_now(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_now(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// W lanes per requested component k: sel [n] its component, out_off [n + 1] its segment of queue / obs_*.  Control flow is uniform
// over the W lanes of a group, so a ballot masked to the group and a shuffle from a lane of the group are well defined.
template <int W>
__global__ __launch_bounds__(TG_BLOCK) void trackgraph_bfs_kernel(int64_t n, const uint32_t *__restrict__ sel, uint32_t attempt,
                                                                  const uint32_t *__restrict__ comp_first, const uint32_t *__restrict__ comp_size,
                                                                  const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ members,
                                                                  const uint32_t *__restrict__ adj_off, const uint32_t *__restrict__ adj,
                                                                  uint32_t *stamp, uint32_t epoch, const int64_t *__restrict__ kp_off, int32_t M,
                                                                  const float *__restrict__ uv, uint32_t *queue, int32_t *__restrict__ obs_img,
                                                                  int32_t *__restrict__ obs_kp, float *__restrict__ obs_uv, uint32_t *err)
{
    const int64_t k = ((int64_t)blockIdx.x * TG_BLOCK + threadIdx.x) / W;
    if (k >= n) return; // the whole group
    const int lane = threadIdx.x & 63, gl = lane & (W - 1);
    const uint64_t gmask = (W == 64 ? ~(uint64_t)0 : (((uint64_t)1 << (W & 63)) - 1)) << (lane & ~(W - 1));
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    const uint32_t c = sel[k], size = comp_size[c], base = out_off[k];
    uint32_t *q = queue + base;
    if (gl == 0) {
        const uint32_t start = members[comp_first[c] + attempt]; // attempt < size: checked on the host
        store_now(&q[0], start);
        store_now(&stamp[start], epoch);
    }
    __threadfence();
    uint32_t head = 0, tail = 1, bad = TG_OK;
    while (head < tail && bad == TG_OK) { // at most `size` pops: tail <= size
        const uint32_t u = load_now(&q[head]);
        ++head;
        const uint32_t beg = adj_off[u], end = adj_off[u + 1];
        for (uint32_t b = beg; b < end; b += W) {
            const uint32_t i = b + (uint32_t)gl;
            const bool valid = i < end;
            const uint32_t d = valid ? adj[i] : 0u;
            const bool unseen = valid && load_now(&stamp[d]) != epoch;
            // equal unseen neighbours resolve to the lowest lane: one round per distinct neighbour, at most W
            uint64_t pending = __ballot(unseen) & gmask;
            bool keep = false;
            while (pending) {
                const int leader = __ffsll((unsigned long long)pending) - 1;
                const uint32_t dl = (uint32_t)__shfl((int)d, leader, 64);
                const uint64_t same = __ballot(unseen && d == dl) & gmask;
                keep = keep || lane == leader;
                pending &= ~same;
            }
            const uint64_t kmask = __ballot(keep) & gmask;
            const uint32_t n_new = (uint32_t)__popcll(kmask);
            if (!tg_append_fits(tail, n_new, size)) { bad = TG_ERR_OVERRUN; break; }
            if (keep) {
                store_now(&q[tail + (uint32_t)__popcll(kmask & below)], d);
                store_now(&stamp[d], epoch);
            }
            tail += n_new;
            __threadfence(); // the next batch and the next pop read what this batch wrote
        }
    }
    if (bad == TG_OK && tail != size) bad = TG_ERR_SHORT;
    if (bad != TG_OK) {
        if (gl == 0) atomicOr(err, bad);
        return;
    }
    for (uint32_t j = (uint32_t)gl; j < size; j += W) {
        const uint32_t node = load_now(&q[j]);
        const int64_t i = tg_owner(kp_off, M - 1, (int64_t)node);
        obs_img[base + j] = (int32_t)i;
        obs_kp[base + j] = (int32_t)((int64_t)node - kp_off[i]);
        if (obs_uv) { obs_uv[2 * (size_t)(base + j)] = uv[2 * (size_t)node]; obs_uv[2 * (size_t)(base + j) + 1] = uv[2 * (size_t)node + 1]; }
    }
}

inline unsigned bits_for(uint64_t largest) { unsigned b = 1; while (b < 64 && (largest >> b)) ++b; return b; }


int32_t build_graph(lvba_trackgraph_s *g, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches)
{
    const int64_t N = g->kp.off.back(), n_matches = n_pairs > 0 ? match_off[n_pairs] : 0;
    lvba_trackgraph_info &info = g->info;
    info.n_skipped = n_matches;
    if (N == 0 || n_matches == 0) return LVBA_OK;
    ScopedStream sg;
    HIPCHK(sg.acquire());
    hipStream_t s = sg.s;

    // ---- half-edges in sequence order, then the adjacency
    std::vector<int64_t> first_seq;
    tg_rank_pairs(n_pairs, pairs, match_off, first_seq);
    const size_t H2 = 2 * (size_t)n_matches;
    const uint32_t no_node = (uint32_t)N;
    const unsigned node_bits = bits_for((uint64_t)N);
    DevArr<int32_t> d_pairs(s); DevArr<int64_t> d_moff(s), d_first(s); DevArr<int32_t> d_matches(s);
    DevArr<uint32_t> d_src(s), d_dst(s), d_key(s);
    HIPCHK(d_pairs.alloc(2 * (size_t)n_pairs)); HIPCHK(d_moff.alloc((size_t)n_pairs + 1)); HIPCHK(d_first.alloc((size_t)n_pairs));
    HIPCHK(d_matches.alloc(2 * (size_t)n_matches)); HIPCHK(d_src.alloc(H2)); HIPCHK(d_dst.alloc(H2)); HIPCHK(d_key.alloc(H2));
    HIPCHK(pool_alloc(&g->d_adj, H2)); HIPCHK(d_pairs.upload(pairs, 2 * (size_t)n_pairs));
    HIPCHK(d_moff.upload(match_off, (size_t)n_pairs + 1)); HIPCHK(d_first.upload(first_seq.data(), (size_t)n_pairs));
    HIPCHK(d_matches.upload(matches, 2 * (size_t)n_matches));
    trackgraph_edge_kernel<<<grid_for(n_matches, TG_BLOCK), TG_BLOCK, 0, s>>>(n_matches, n_pairs, d_pairs, d_moff,
                                                                            d_first, d_matches, g->kp.d_off, no_node,
                                                                            d_src, d_dst);
    HIPCHK(hipGetLastError());
    TRY(sort_pairs<uint32_t>(s, d_src, d_key, d_dst, g->d_adj, H2, node_bits)); HIPCHK(pool_alloc(&g->d_adj_off, ((size_t)N + 1)));
    trackgraph_offsets_kernel<<<grid_for(N + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(N, d_key, (uint32_t)H2, g->d_adj_off);
    HIPCHK(hipGetLastError());
    uint32_t n_half = 0;
    HIPCHK(hipMemcpyAsync(&n_half, g->d_adj_off + N, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    info.n_edges = n_half / 2;
    info.n_skipped = n_matches - info.n_edges;
    if (n_half == 0) return LVBA_OK;

    // ---- labels
    DevArr<uint32_t> d_label(s), d_changed(s);
    HIPCHK(d_label.alloc((size_t)N)); HIPCHK(d_changed.alloc(1));
    trackgraph_iota_kernel<<<grid_for(N, TG_BLOCK), TG_BLOCK, 0, s>>>(N, d_label);
    HIPCHK(hipGetLastError());
    int rounds = 0;
    for (uint32_t changed = 1; changed;) {
        if (rounds == TG_MAX_ROUNDS) return lvba_fail(LVBA_ERR_STATE, "the component labels did not settle in %d rounds", TG_MAX_ROUNDS);
        ++rounds;
        HIPCHK(d_changed.zero_async(1));
        trackgraph_hook_kernel<<<grid_for(n_half, TG_BLOCK), TG_BLOCK, 0, s>>>(n_half, d_key, g->d_adj, d_label,
                                                                             d_changed);
        HIPCHK(hipGetLastError());
        trackgraph_jump_kernel<<<grid_for(N, TG_BLOCK), TG_BLOCK, 0, s>>>(N, d_label, d_changed);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&changed, d_changed, d_changed.bytes(1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    info.cc_rounds = rounds;

    // ---- the nodes with an edge, by (label, node)
    DevArr<uint32_t> d_flag(s), d_excl(s), d_node(s), d_node_label(s), d_lab(s);
    HIPCHK(d_flag.alloc((size_t)N + 1)); HIPCHK(d_excl.alloc((size_t)N + 1));
    trackgraph_degree_kernel<<<grid_for(N + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(N, g->d_adj_off, d_flag);
    HIPCHK(hipGetLastError());
    int64_t n_nodes = 0;
    TRY(count_flags(s, d_flag, d_excl, (size_t)N + 1, &n_nodes));
    info.n_nodes = n_nodes;
    HIPCHK(d_node.alloc((size_t)n_nodes)); HIPCHK(d_node_label.alloc((size_t)n_nodes)); HIPCHK(d_lab.alloc((size_t)n_nodes));
    HIPCHK(pool_alloc(&g->d_members, (size_t)n_nodes));
    trackgraph_nodes_kernel<<<grid_for(N, TG_BLOCK), TG_BLOCK, 0, s>>>(N, d_flag, d_excl, d_label,
                                                                     d_node, d_node_label);
    HIPCHK(hipGetLastError());
    TRY(sort_pairs<uint32_t>(s, d_node_label, d_lab, d_node, g->d_members, (size_t)n_nodes, node_bits));

    // ---- runs, sizes, distinct images, the two checks, the table
    DevArr<int32_t> d_img(s); DevArr<uint32_t> d_head(s), d_change(s), d_run_of(s), d_change_x(s), d_run_first(s);
    HIPCHK(d_img.alloc((size_t)n_nodes)); HIPCHK(d_head.alloc((size_t)n_nodes + 1)); HIPCHK(d_change.alloc((size_t)n_nodes + 1));
    HIPCHK(d_run_of.alloc((size_t)n_nodes + 1)); HIPCHK(d_change_x.alloc((size_t)n_nodes + 1));
    trackgraph_image_kernel<<<grid_for(n_nodes, TG_BLOCK), TG_BLOCK, 0, s>>>(n_nodes, g->d_members, g->kp.d_off, g->kp.n_images, d_img);
    HIPCHK(hipGetLastError());
    trackgraph_runs_kernel<<<grid_for(n_nodes + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(n_nodes, d_lab, d_img,
                                                                              d_head, d_change);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, d_head, d_run_of, (size_t)n_nodes + 1));
    TRY(scan_excl<uint32_t>(s, d_change, d_change_x, (size_t)n_nodes + 1));
    uint32_t n_all = 0;
    HIPCHK(copy_d2h(&n_all, d_run_of + n_nodes, d_run_of.bytes(1)));
    info.n_components_all = n_all;
    HIPCHK(d_run_first.alloc((size_t)n_all + 1));
    trackgraph_heads_kernel<<<grid_for(n_nodes + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(n_nodes, d_head, d_run_of,
                                                                               d_run_first);
    HIPCHK(hipGetLastError());
    DevArr<uint32_t> d_keep(s), d_kept_size(s), d_comp_of(s), d_obs_x(s), d_comp_images(s);
    HIPCHK(d_keep.alloc((size_t)n_all + 1)); HIPCHK(d_kept_size.alloc((size_t)n_all + 1));
    HIPCHK(d_comp_of.alloc((size_t)n_all + 1)); HIPCHK(d_obs_x.alloc((size_t)n_all + 1));
    trackgraph_check_kernel<<<grid_for((int64_t)n_all + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(n_all, d_run_first, d_change_x,
                                                                                      g->obser_thr, d_keep, d_kept_size);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, d_keep, d_comp_of, (size_t)n_all + 1));
    TRY(scan_excl<uint32_t>(s, d_kept_size, d_obs_x, (size_t)n_all + 1));
    uint32_t n_comp = 0;
    HIPCHK(copy_d2h(&n_comp, d_comp_of + n_all, d_comp_of.bytes(1)));
    info.n_components = n_comp;
    HIPCHK(pool_alloc(&g->d_comp_first, (size_t)n_comp)); HIPCHK(pool_alloc(&g->d_comp_size, (size_t)n_comp));
    HIPCHK(pool_alloc(&g->d_comp_obs, ((size_t)n_comp + 1))); HIPCHK(d_comp_images.alloc((size_t)n_comp));
    trackgraph_table_kernel<<<grid_for((int64_t)n_all + 1, TG_BLOCK), TG_BLOCK, 0, s>>>(n_all, d_run_first, d_change_x,
                                                                                      d_keep, d_comp_of, d_obs_x,
                                                                                      g->d_comp_first, g->d_comp_size, d_comp_images,
                                                                                      g->d_comp_obs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    g->comp_size.resize(n_comp); g->comp_images.resize(n_comp);
    if (n_comp > 0) {
        HIPCHK(lvba::copy_d2h(g->comp_size.data(), g->d_comp_size, 4 * (size_t)n_comp));
        HIPCHK(d_comp_images.download(g->comp_images.data(), (size_t)n_comp));
    }
    for (uint32_t sz : g->comp_size) {
        info.n_observations += sz;
        info.largest_component = std::max<int64_t>(info.largest_component, sz);
    }
    HIPCHK(pool_alloc(&g->d_stamp, (size_t)N));
    HIPCHK(hipMemsetAsync(g->d_stamp, 0, 4 * (size_t)N, s));
    HIPCHK(hipStreamSynchronize(s));
    return LVBA_OK;
}

} // namespace

extern "C" int32_t lvba_trackgraph_destroy(lvba_trackgraph_t g)
{
    if (!g) return LVBA_OK;
    (void)hipSetDevice(g->kp.device);
    (void)hipDeviceSynchronize();
    image_set_free(g->kp);
    for (void *p : {(void *)g->d_adj_off, (void *)g->d_adj, (void *)g->d_members, (void *)g->d_stamp,
                    (void *)g->d_comp_first, (void *)g->d_comp_size, (void *)g->d_comp_obs})
        if (p) DevicePool::get().free(p);
    delete g;
    return LVBA_OK;
}

extern "C" int32_t lvba_trackgraph_create(int32_t device, int32_t n_images, const int64_t *kp_off, const float *keypoints_uv, int64_t n_pairs,
                                          const int32_t *pairs, const int64_t *match_off, const int32_t *matches, int32_t obser_thr,
                                          lvba_trackgraph_t *out, lvba_trackgraph_info *info)
{
    if (!out || !kp_off || n_images < 0 || n_pairs < 0) return lvba_fail(LVBA_ERR_ARG, "null argument or a negative count");
    if (n_pairs > 0 && (!pairs || !match_off)) return lvba_fail(LVBA_ERR_ARG, "null pairs or match_off");
    if (obser_thr < 1) return lvba_fail(LVBA_ERR_ARG, "obser_thr = %d (>= 1)", obser_thr);
    TRY(check_offsets("kp_off", "image", n_images, kp_off));
    if (kp_off[n_images] >= TG_MAX_NODES)
        return lvba_fail(LVBA_ERR_UNSUPPORTED, "%lld key points (fewer than 2^31: node ids are 32 bits)", (long long)kp_off[n_images]);
    const int64_t n_matches = n_pairs > 0 ? match_off[n_pairs] : 0;
    if (n_pairs > 0) {
        TRY(check_offsets("match_off", "pair", n_pairs, match_off));
        if (n_matches >= TG_MAX_MATCHES)
            return lvba_fail(LVBA_ERR_UNSUPPORTED, "%lld matches (fewer than 2^30: half-edge ids are 32 bits)", (long long)n_matches);
        for (int64_t p = 0; p < n_pairs; ++p) TRY(check_image_pair(pairs[2 * p], pairs[2 * p + 1], n_images));
        if (n_matches > 0 && !matches) return lvba_fail(LVBA_ERR_ARG, "null matches");
    }
    TRY(check_device(device));
    HIPCHK(hipSetDevice(device));
    lvba_trackgraph_s *g = new lvba_trackgraph_s;
    g->kp = ImageSet{device, n_images, std::vector<int64_t>(kp_off, kp_off + n_images + 1)};
    g->obser_thr = obser_thr; g->has_uv = keypoints_uv != nullptr;
    int32_t rc = image_set_upload(g->kp, true, keypoints_uv);
    if (rc == LVBA_OK) rc = build_graph(g, n_pairs, pairs, match_off, matches);
    if (rc != LVBA_OK) { lvba_trackgraph_destroy(g); return rc; }
    if (info) *info = g->info;
    *out = g;
    return LVBA_OK;
}

extern "C" int32_t lvba_trackgraph_components(lvba_trackgraph_t g, int64_t *comp_off, int32_t *mem_img, int32_t *mem_kp, int32_t *comp_images)
{
    if (!g || !comp_off) return lvba_fail(LVBA_ERR_ARG, "null handle or comp_off");
    const int64_t n_obs = g->info.n_observations, n_comp = g->info.n_components;
    if (n_obs > 0 && (!mem_img || !mem_kp)) return lvba_fail(LVBA_ERR_ARG, "null mem_img or mem_kp");
    if (n_obs > 0) {
        HIPCHK(hipSetDevice(g->kp.device));
        ScopedStream sg;
        HIPCHK(sg.acquire());
        DevArr<int32_t> d_img(sg.s), d_kp(sg.s);
        HIPCHK(d_img.alloc((size_t)n_obs)); HIPCHK(d_kp.alloc((size_t)n_obs));
        trackgraph_members_kernel<<<grid_for(n_obs, TG_BLOCK), TG_BLOCK, 0, sg.s>>>(n_obs, (uint32_t)n_comp, g->d_comp_obs, g->d_comp_first, g->d_members,
                                                                                 g->kp.d_off, g->kp.n_images, d_img, d_kp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(sg.s));
        HIPCHK(d_img.download(mem_img, (size_t)n_obs)); HIPCHK(d_kp.download(mem_kp, (size_t)n_obs));
    }
    comp_off[0] = 0;
    for (int64_t c = 0; c < n_comp; ++c) {
        comp_off[c + 1] = comp_off[c] + g->comp_size[(size_t)c];
        if (comp_images) comp_images[c] = (int32_t)g->comp_images[(size_t)c];
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_trackgraph_orders(lvba_trackgraph_t g, int64_t n, const int64_t *comp, int32_t attempt, int64_t *obs_off, int32_t *obs_img,
                                          int32_t *obs_kp, float *obs_uv)
{
    if (!g || !obs_off || n < 0 || attempt < 0) return lvba_fail(LVBA_ERR_ARG, "null handle or obs_off, n < 0 or attempt < 0");
    const int64_t n_comp = g->info.n_components;
    if (!comp && n != n_comp) return lvba_fail(LVBA_ERR_ARG, "comp = NULL asks for all %lld components, n = %lld", (long long)n_comp, (long long)n);
    if (obs_uv && !g->has_uv) return lvba_fail(LVBA_ERR_ARG, "obs_uv asked of a graph that was created without key points");
    std::vector<uint32_t> sel((size_t)n), off((size_t)n + 1, 0u);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t c = comp ? comp[k] : k;
        if (c < 0 || c >= n_comp || (k > 0 && c <= (int64_t)sel[(size_t)k - 1]))
            return lvba_fail(LVBA_ERR_ARG, "comp[%lld] = %lld: strictly ascending in [0, %lld)", (long long)k, (long long)c, (long long)n_comp);
        if ((uint32_t)attempt >= g->comp_size[(size_t)c])
            return lvba_fail(LVBA_ERR_ARG, "attempt %d of component %lld, which has %u members", attempt, (long long)c, g->comp_size[(size_t)c]);
        sel[(size_t)k] = (uint32_t)c;
        off[(size_t)k + 1] = off[(size_t)k] + g->comp_size[(size_t)c];
    }
    const size_t total = off[(size_t)n];
    if (total > 0 && (!obs_img || !obs_kp)) return lvba_fail(LVBA_ERR_ARG, "null obs_img or obs_kp");
    if (total > 0) {
        HIPCHK(hipSetDevice(g->kp.device));
        ScopedStream sg;
        HIPCHK(sg.acquire());
        hipStream_t s = sg.s;
        if (++g->epoch == 0) { // every stamp of 2^32 calls ago is stale by now
            HIPCHK(hipMemsetAsync(g->d_stamp, 0, 4 * (size_t)g->kp.off.back(), s));
            g->epoch = 1;
        }
        DevArr<uint32_t> d_sel(s), d_off(s), d_queue(s); DevArr<int32_t> d_img(s), d_kp(s); DevArr<float> d_uv(s);
        DevArr<uint32_t> d_err(s);
        HIPCHK(d_sel.alloc((size_t)n)); HIPCHK(d_off.alloc((size_t)n + 1)); HIPCHK(d_queue.alloc(total));
        HIPCHK(d_img.alloc(total)); HIPCHK(d_kp.alloc(total)); HIPCHK(d_err.alloc(1));
        if (obs_uv) HIPCHK(d_uv.alloc(2 * total));
        HIPCHK(d_sel.upload(sel.data(), (size_t)n)); HIPCHK(d_off.upload(off.data(), (size_t)n + 1)); HIPCHK(d_err.zero_async(1));
        trackgraph_bfs_kernel<TG_BFS_LANES><<<grid_for(n * TG_BFS_LANES, TG_BLOCK), TG_BLOCK, 0, s>>>(
            n, d_sel, (uint32_t)attempt, g->d_comp_first, g->d_comp_size, d_off, g->d_members, g->d_adj_off, g->d_adj,
            g->d_stamp, g->epoch, g->kp.d_off, g->kp.n_images, g->kp.d_uv, d_queue, d_img, d_kp,
            obs_uv ? d_uv : nullptr, d_err);
        HIPCHK(hipGetLastError());
        uint32_t err = 0;
        HIPCHK(hipMemcpyAsync(&err, d_err, d_err.bytes(1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (err) return lvba_fail(LVBA_ERR_STATE, "a breadth-first walk ended %s its component's size", err & TG_ERR_OVERRUN ? "beyond" : "short of");
        HIPCHK(d_img.download(obs_img, total)); HIPCHK(d_kp.download(obs_kp, total));
        if (obs_uv) HIPCHK(d_uv.download(obs_uv, 2 * total));
    }
    for (int64_t k = 0; k <= n; ++k) obs_off[k] = off[(size_t)k];
    return LVBA_OK;
}
