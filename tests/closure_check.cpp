// closure_check.cpp -- csrc/closure_device.h compiled for the host (tests/test_closure_host.py): the pair test over all pairs and
// the set search in plain loops, with the header's own arithmetic, decisions, orders and bit-set steps.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/closure_device.h"

using namespace lvba;

extern "C" {

// X [n_frames][12], Z [M][12], tol = {rot_tol, rot_rate, trans_tol, trans_rate}; adj [M][W], rot, trans [M][M]
void emul_adjacency(const double *X, int M, const int32_t *ref, const int32_t *query, const double *Z, const double *tol, uint64_t *adj,
                    double *rot, double *trans)
{
    ClosureParams o;
    o.rot_tol = tol[0]; o.rot_rate = tol[1]; o.trans_tol = tol[2]; o.trans_rate = tol[3];
    const int W = (M + 63) / 64;
    std::vector<double> prep((size_t)CLOSURE_PREP * M);
    for (int k = 0; k < M; ++k) closure_prepare(X + 12 * (size_t)ref[k], X + 12 * (size_t)query[k], Z + 12 * (size_t)k, &prep[(size_t)CLOSURE_PREP * k]);
    for (size_t e = 0; e < (size_t)M * W; ++e) adj[e] = 0;
    for (int a = 0; a < M; ++a)
        for (int b = 0; b < M; ++b) {
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            double r = 0.0, t = 0.0;
            bool ok = true;
            if (a != b) {
                closure_measures(&prep[(size_t)CLOSURE_PREP * lo], &prep[(size_t)CLOSURE_PREP * hi], &r, &t);
                ok = closure_consistent(r, t, closure_path(ref[lo], query[lo], ref[hi], query[hi]), o);
            }
            rot[(size_t)a * M + b] = r; trans[(size_t)a * M + b] = t;
            if (ok) adj[(size_t)a * W + (b >> 6)] |= (uint64_t)1 << (b & 63);
        }
}

// adj [M][W]; seeds [min(n_seeds, M)]; picks [min(n_seeds, M)][M] with n_picks of them per seed (the rounds; with `shortcut` only
// those before C was found to be a clique); sets [min(n_seeds, M)][W]; keep [M]; returns n_keep
int32_t emul_set(int M, const uint64_t *adj, int n_seeds, int min_set, int shortcut, int32_t *deg, int32_t *seeds, int32_t *picks,
                 int32_t *n_picks, uint64_t *sets, uint8_t *keep)
{
    const int W = (M + 63) / 64, ns = n_seeds < M ? n_seeds : M;
    for (int v = 0; v < M; ++v) deg[v] = closure_row_bits(adj + (size_t)v * W, 0, W, 1) - 1;
    for (int v = 0; v < M; ++v) {
        int rank = 0;
        for (int u = 0; u < M; ++u) rank += closure_before(deg[u], u, deg[v], v) ? 1 : 0;
        if (rank < ns) seeds[rank] = v;
    }
    int32_t best_size = -1, best = INT32_MAX;
    std::vector<uint64_t> C(W);
    for (int k = 0; k < ns; ++k) {
        const int32_t s = seeds[k];
        uint64_t *K = sets + (size_t)k * W;
        for (int w = 0; w < W; ++w) {
            C[w] = closure_take(adj[(size_t)s * W + w], ~(uint64_t)0, w, s);
            K[w] = closure_bit(w, s);
        }
        int csize = deg[s], ksize = 1;
        n_picks[k] = 0;
        while (csize > 0) {
            int32_t bc = -1, bv = INT32_MAX;
            bool all = true;
            for (int w = 0; w < W; ++w)
                for (uint64_t word = C[w]; word; word &= word - 1) {
                    const int32_t v = 64 * w + __builtin_ctzll(word);
                    const int32_t cnt = closure_row_count(adj + (size_t)v * W, C.data(), 0, W, 1);
                    if (closure_before(cnt, v, bc, bv)) { bc = cnt; bv = v; }
                    all = all && cnt == csize;
                }
            if (shortcut && all) {
                for (int w = 0; w < W; ++w) K[w] |= C[w];
                ksize += csize;
                break;
            }
            picks[(size_t)k * M + n_picks[k]++] = bv;
            for (int w = 0; w < W; ++w) {
                C[w] = closure_take(C[w], adj[(size_t)bv * W + w], w, bv);
                K[w] |= closure_bit(w, bv);
            }
            csize = bc - 1;
            ++ksize;
        }
        if (closure_before(ksize, k, best_size, best)) { best_size = ksize; best = k; }
    }
    const bool any = ns > 0 && best_size >= min_set;
    for (int v = 0; v < M; ++v) keep[v] = any && ((sets[(size_t)best * W + (v >> 6)] >> (v & 63)) & 1) ? 1 : 0;
    return any ? best_size : 0;
}

} // extern "C"
