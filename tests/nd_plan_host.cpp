// The nested-dissection plan a handle would take for a pose graph, computed on the host (global-lvba_amd/csrc/nd_plan.h is
// host-only): what lets tests/test_nd_reference_host.py choose and check rows without a GPU, and what tests/test_gpu_nd_edges.py
// holds a handle's exported partition to.  The choice of the band ordering repeats bs_build (block_system.hip): the natural
// order's block half-bandwidth against rcm_order's, the smaller wins (ties: the natural order); then nd_plan with
// min_gain = 1e30, which is what LVBA_SOLVER=nd does.
#include <cstdlib>
#include <cstring>
#include <string>
#include "../global-lvba_amd/csrc/nd_plan.h"

// adj [N][N] bytes (symmetric); chunk_ranks > 0: LVBA_ND_CHUNK_RANKS for the duration of the call (restored afterwards), else unset.
// head [8]: active, kind (0 band, 1 hubs, 2 chunks), ps, Ns, BbS, arcs, Bb of the band ordering, 1 if that ordering is rcm_order's.
// perm_band [N]: that ordering; perm [N]: the plan's (the band ordering again if the band is kept); arcs [arcs][4]: p0, Na, Bb, owner; sep_off [arcs + 1] into sep (separator-local poses, ascending).
// Returns 0, or 1 if max_arcs / sep_cap are too small (head is filled either way; head[5] and the return of a second call say how much).
extern "C" int nd_plan_host(const uint8_t *adj, int32_t N, int32_t n_ranks, int32_t chunk_ranks, int32_t *head, int32_t *perm_band, int32_t *perm,
                            int32_t *arcs, int32_t max_arcs, int32_t *sep_off, int32_t *sep, int64_t sep_cap)
{
    const char *name = "LVBA_ND_CHUNK_RANKS";
    const char *old = getenv(name);
    const std::string keep = old ? old : "";
    if (chunk_ranks > 0) setenv(name, std::to_string(chunk_ranks).c_str(), 1);
    else unsetenv(name);

    lvba::hvec<uint8_t> a(adj, adj + (size_t)N * N);
    lvba::hvec<int32_t> band((size_t)N), rcm, ircm((size_t)N);
    for (int i = 0; i < N; ++i) band[(size_t)i] = i;
    lvba::rcm_order(a, N, rcm);
    for (int i = 0; i < N; ++i) ircm[(size_t)rcm[(size_t)i]] = i;
    int32_t Bb_nat = 0, Bb_rcm = 0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (a[(size_t)i * N + j] && i != j) {
                Bb_nat = std::max(Bb_nat, std::abs(i - j));
                Bb_rcm = std::max(Bb_rcm, std::abs(ircm[(size_t)i] - ircm[(size_t)j]));
            }
    const bool use_rcm = Bb_rcm < Bb_nat;
    if (use_rcm) band = rcm;
    const int32_t Bb = use_rcm ? Bb_rcm : Bb_nat;
    const lvba::NdPlan pl = lvba::nd_plan(a.data(), N, band, Bb, n_ranks, 1e30);

    if (old) setenv(name, keep.c_str(), 1);
    else unsetenv(name);

    head[0] = pl.active ? 1 : 0;
    head[1] = !pl.active ? 0 : !std::strcmp(pl.kind, "hubs") ? 1 : 2;
    head[2] = pl.ps; head[3] = pl.Ns; head[4] = pl.BbS; head[5] = (int32_t)pl.arcs.size();
    head[6] = Bb; head[7] = use_rcm ? 1 : 0;
    for (int i = 0; i < N; ++i) perm_band[i] = band[(size_t)i];
    for (int i = 0; i < N; ++i) perm[i] = pl.active ? pl.perm[(size_t)i] : band[(size_t)i];
    if ((int32_t)pl.arcs.size() > max_arcs) return 1;
    int64_t at = 0;
    for (size_t k = 0; k < pl.arcs.size(); ++k) {
        const lvba::NdPlanArc &A = pl.arcs[k];
        arcs[4 * k + 0] = A.p0; arcs[4 * k + 1] = A.Na; arcs[4 * k + 2] = A.Bb; arcs[4 * k + 3] = A.owner;
        sep_off[k] = (int32_t)at;
        if (at + (int64_t)A.sep.size() > sep_cap) return 1;
        for (int32_t q : A.sep) sep[at++] = q;
    }
    sep_off[pl.arcs.size()] = (int32_t)at;
    return 0;
}
