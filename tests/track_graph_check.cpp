// track_graph_check.cpp -- csrc/track_graph_device.h compiled for the host behind a stand-alone driver (tests/test_track_graph_host.py):
// the half-edge placement, the label rounds, the member and threshold pass and the BFS walker, walked the way the kernels of
// track_graph.hip walk them (the BFS with its batches of `lanes` neighbours), with the header's own functions.  A program, not a
// library, so that the build with -fsanitize=address,undefined runs as it is.  TEST INFRASTRUCTURE ONLY.
//   track_graph_check IN OUT     IN / OUT: int64 streams, little endian
//   IN : M, kp_off [M + 1], n_pairs, pairs [n_pairs][2], match_off [n_pairs + 1], matches [.][2], obser_thr, lanes, n_attempts, attempts []
//   OUT: n_nodes, n_edges, n_skipped, n_components_all, n_components, n_observations, largest_component, rounds,
//        adj_off [N + 1], adj [2 n_edges], comp_off [n_components + 1], mem_img [], mem_kp [], comp_images [n_components], then per
//        attempt a: n_sel, sel [] (the components with more than a members), obs_off [n_sel + 1], obs_img [], obs_kp []
// Exit status 0, or 2 when the two label schedules disagree, 3 when the rounds pass their cap, 4 when a walk misses its size.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../global-lvba_amd/csrc/track_graph_device.h"

using namespace lvba;

namespace {

struct Reader {
    std::vector<int64_t> v;
    size_t at = 0;
    int64_t one() { return at < v.size() ? v[at++] : 0; }
    template <class T> std::vector<T> many(int64_t n)
    {
        std::vector<T> out((size_t)n);
        for (auto &x : out) x = (T)one();
        return out;
    }
};

// the label rounds with the half-edges taken forwards or backwards: the fixed point must not depend on it
int label_rounds(const std::vector<uint32_t> &key, const std::vector<uint32_t> &adj, uint32_t n_half, int64_t N, bool backwards,
                 std::vector<uint32_t> &label)
{
    label.resize((size_t)N);
    for (int64_t v = 0; v < N; ++v) label[(size_t)v] = (uint32_t)v;
    int rounds = 0;
    for (bool changed = n_half > 0; changed;) { // no edge, no round: as lvba_trackgraph_create
        if (rounds == TG_MAX_ROUNDS) return -1;
        ++rounds;
        changed = false;
        for (uint32_t k = 0; k < n_half; ++k) {
            const uint32_t i = backwards ? n_half - 1 - k : k;
            changed = tg_hook(label.data(), key[i], adj[i]) || changed;
        }
        for (int64_t k = 0; k < N; ++k) changed = tg_jump(label.data(), (uint32_t)(backwards ? N - 1 - k : k)) || changed;
    }
    return rounds;
}

// trackgraph_bfs_kernel for one component: W lanes, the segment q [size] is the queue
uint32_t bfs_walk(int W, uint32_t start, uint32_t size, const std::vector<uint32_t> &adj_off, const std::vector<uint32_t> &adj,
                  std::vector<uint32_t> &stamp, uint32_t epoch, uint32_t *q)
{
    q[0] = start; stamp[start] = epoch;
    uint32_t head = 0, tail = 1;
    std::vector<uint32_t> d((size_t)W);
    std::vector<char> unseen((size_t)W), keep((size_t)W);
    while (head < tail) {
        const uint32_t u = q[head++];
        for (uint32_t b = adj_off[u]; b < adj_off[u + 1]; b += (uint32_t)W) {
            for (int l = 0; l < W; ++l) {
                const uint32_t i = b + (uint32_t)l;
                const bool valid = i < adj_off[u + 1];
                d[(size_t)l] = valid ? adj[i] : 0u;
                unseen[(size_t)l] = valid && stamp[d[(size_t)l]] != epoch;
                keep[(size_t)l] = 0;
            }
            std::vector<char> pending(unseen);
            for (int leader = 0; leader < W; ++leader) { // the lowest pending lane leads; the lanes that hold its neighbour retire
                if (!pending[(size_t)leader]) continue;
                keep[(size_t)leader] = 1;
                for (int l = leader; l < W; ++l)
                    if (unseen[(size_t)l] && d[(size_t)l] == d[(size_t)leader]) pending[(size_t)l] = 0;
            }
            uint32_t n_new = 0;
            for (int l = 0; l < W; ++l) n_new += keep[(size_t)l] ? 1u : 0u;
            if (!tg_append_fits(tail, n_new, size)) return TG_ERR_OVERRUN;
            for (int l = 0; l < W; ++l)
                if (keep[(size_t)l]) { q[tail++] = d[(size_t)l]; stamp[d[(size_t)l]] = epoch; }
        }
    }
    return tail == size ? TG_OK : TG_ERR_SHORT;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    Reader in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 1;
        int64_t x;
        while (fread(&x, 8, 1, f) == 1) in.v.push_back(x);
        fclose(f);
    }
    const int64_t M = in.one();
    const std::vector<int64_t> kp_off = in.many<int64_t>(M + 1);
    const int64_t n_pairs = in.one();
    const std::vector<int32_t> pairs = in.many<int32_t>(2 * n_pairs);
    const std::vector<int64_t> match_off = in.many<int64_t>(n_pairs + 1);
    const int64_t n_matches = match_off[(size_t)n_pairs];
    const std::vector<int32_t> matches = in.many<int32_t>(2 * n_matches);
    const int32_t thr = (int32_t)in.one();
    const int W = (int)in.one();
    const std::vector<int64_t> attempts = in.many<int64_t>(in.one());
    const int64_t N = kp_off[(size_t)M];
    std::vector<int64_t> out;

    // half-edges (trackgraph_edge_kernel), a stable sort by src, the offsets (trackgraph_offsets_kernel)
    const size_t H2 = 2 * (size_t)n_matches;
    std::vector<int64_t> first_seq;
    tg_rank_pairs(n_pairs, pairs.data(), match_off.data(), first_seq);
    std::vector<uint32_t> src(H2), dst(H2), key(H2), adj(H2);
    for (int64_t row = 0; row < n_matches; ++row)
        tg_half_edges(row, n_pairs, pairs.data(), match_off.data(), first_seq.data(), matches.data(), kp_off.data(), (uint32_t)N, src.data(), dst.data());
    {
        std::vector<uint32_t> idx(H2);
        std::iota(idx.begin(), idx.end(), 0u);
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return src[a] < src[b]; });
        for (size_t i = 0; i < H2; ++i) { key[i] = src[idx[i]]; adj[i] = dst[idx[i]]; }
    }
    std::vector<uint32_t> adj_off((size_t)N + 1);
    for (int64_t v = 0; v <= N; ++v) adj_off[(size_t)v] = tg_lower_bound(key.data(), (uint32_t)H2, (uint32_t)v);
    const uint32_t n_half = adj_off[(size_t)N];

    // labels (trackgraph_hook_kernel, trackgraph_jump_kernel), under two schedules
    std::vector<uint32_t> label, other;
    const int rounds = label_rounds(key, adj, n_half, N, false, label);
    if (rounds < 0 || label_rounds(key, adj, n_half, N, true, other) < 0) return 3;
    if (label != other) return 2;

    // the nodes with an edge by (label, node), runs, sizes, distinct images, the two checks (trackgraph_nodes_kernel .. _table_kernel)
    std::vector<uint32_t> members, lab;
    {
        std::vector<uint32_t> node;
        for (int64_t v = 0; v < N; ++v)
            if (adj_off[(size_t)v + 1] > adj_off[(size_t)v]) node.push_back((uint32_t)v);
        std::stable_sort(node.begin(), node.end(), [&](uint32_t a, uint32_t b) { return label[a] < label[b]; });
        members = node;
        for (uint32_t v : members) lab.push_back(label[v]);
    }
    const int64_t n_nodes = (int64_t)members.size();
    std::vector<int32_t> img((size_t)n_nodes);
    for (int64_t i = 0; i < n_nodes; ++i) img[(size_t)i] = (int32_t)tg_owner(kp_off.data(), M - 1, members[(size_t)i]);
    std::vector<uint32_t> run_first, change_x((size_t)n_nodes + 1, 0u);
    for (int64_t i = 0; i < n_nodes; ++i) {
        if (tg_run_head(lab.data(), i)) run_first.push_back((uint32_t)i);
        change_x[(size_t)i + 1] = change_x[(size_t)i] + (tg_image_change(lab.data(), img.data(), i) ? 1u : 0u);
    }
    const int64_t n_all = (int64_t)run_first.size();
    run_first.push_back((uint32_t)n_nodes);
    std::vector<uint32_t> comp_first, comp_size, comp_images;
    for (int64_t r = 0; r < n_all; ++r) {
        const uint32_t a = run_first[(size_t)r], b = run_first[(size_t)r + 1];
        if (!tg_qualifies(b - a, change_x[b] - change_x[a], thr)) continue;
        comp_first.push_back(a); comp_size.push_back(b - a); comp_images.push_back(change_x[b] - change_x[a]);
    }
    const int64_t n_comp = (int64_t)comp_size.size();
    int64_t n_obs = 0, largest = 0;
    for (uint32_t s : comp_size) { n_obs += s; largest = std::max<int64_t>(largest, s); }
    for (int64_t x : {n_nodes, (int64_t)n_half / 2, n_matches - (int64_t)n_half / 2, n_all, n_comp, n_obs, largest, (int64_t)rounds}) out.push_back(x);
    for (uint32_t x : adj_off) out.push_back(x);
    for (uint32_t i = 0; i < n_half; ++i) out.push_back(adj[i]);
    int64_t off = 0;
    out.push_back(0);
    for (uint32_t s : comp_size) out.push_back(off += s);
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t c = 0; c < n_comp; ++c)
            for (uint32_t k = 0; k < comp_size[(size_t)c]; ++k) {
                const uint32_t node = members[comp_first[(size_t)c] + k];
                const int64_t i = tg_owner(kp_off.data(), M - 1, node);
                out.push_back(pass == 0 ? i : (int64_t)node - kp_off[(size_t)i]);
            }
    for (uint32_t x : comp_images) out.push_back(x);

    // the orders (trackgraph_bfs_kernel): every segment is exactly its component's size, so an overrun is a heap overrun here
    std::vector<uint32_t> stamp((size_t)N, 0u);
    uint32_t epoch = 0;
    for (int64_t a : attempts) {
        ++epoch;
        std::vector<int64_t> sel;
        for (int64_t c = 0; c < n_comp; ++c)
            if ((int64_t)comp_size[(size_t)c] > a) sel.push_back(c);
        out.push_back((int64_t)sel.size());
        for (int64_t c : sel) out.push_back(c);
        std::vector<std::vector<uint32_t>> q(sel.size());
        int64_t at = 0;
        out.push_back(0);
        for (size_t k = 0; k < sel.size(); ++k) {
            const int64_t c = sel[k];
            q[k].resize(comp_size[(size_t)c]);
            if (bfs_walk(W, members[comp_first[(size_t)c] + (uint32_t)a], comp_size[(size_t)c], adj_off, adj, stamp, epoch, q[k].data()) != TG_OK) return 4;
            out.push_back(at += comp_size[(size_t)c]);
        }
        for (int pass = 0; pass < 2; ++pass)
            for (auto &qq : q)
                for (uint32_t node : qq) {
                    const int64_t i = tg_owner(kp_off.data(), M - 1, node);
                    out.push_back(pass == 0 ? i : (int64_t)node - kp_off[(size_t)i]);
                }
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = out.empty() || fwrite(out.data(), 8, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 1;
}
