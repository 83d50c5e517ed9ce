// prior_tables.h -- the host side of the pose priors that both stages share (lvba_balm_set_priors, lvba_visual_set_priors): the
// argument checks, the stored copy, and the binding of the priors to the solver order -- the PriorRec records and the CSR scatter
// tables of prior_scatter_kernel (priors.hip) with their device copies.  What differs between the stages stays in their API files:
// which blocks hold something besides priors, and what happens after a failed binding.
#pragma once
#include <vector>
#include "block_system.h"

namespace lvba {

// A handle's priors on the device.  Between release() and a successful bind() dev.n == 0: a handle without priors.
struct PriorTables {
    PriorDev dev;
    std::vector<void *> mem;     // device allocations behind dev and d_wslot
    int64_t *d_wslot = nullptr;  // blocks that only priors fill: zeroed when the priors are replaced
    int64_t n_wslot = 0;

    // zero the write-only blocks on bs.stream, free the allocations, reset
    int32_t release(BlockSys &bs);
    // (after release, the store laid out) priors -> records in solver order, scatter tables, device copies.  other_slots (sorted):
    // the blocks that hold something besides priors -- a prior adds to those and to the diagonal, and writes the others; all_add:
    // every block is added to.  n_sums: partial sums per workgroup of the stage's grid sums.  offdiag (may be NULL): receives the
    // slots of the off-diagonal blocks.
    int32_t bind(BlockSys &bs, const std::vector<lvba_prior> &priors, const lvba::hvec<int64_t> &other_slots, bool all_add, int n_sums,
                 lvba::hvec<int64_t> *offdiag);
    void free_mem(); // (a handle's destructor: no stream work)
};

// the steps of lvba_*_set_priors
int32_t prior_cap(int32_t n); // at most 2^22 priors
// a laid-out store: every RELATIVE pair must be one of its blocks -- inside the band and, when lists are given (sorted; each may be
// NULL), in one of them.  what / call: "poses", "eval" or "cameras", "linearize" (the message)
int32_t prior_pairs_in_store(const BlockSys &bs, int32_t n, const lvba_prior *priors, const lvba::hvec<int64_t> *slots_a,
                             const lvba::hvec<int64_t> *slots_b, const char *what, const char *call);
// stored <- the priors with the fields their kind does not use zeroed (prior_hash compares bytes); before the store is laid out
// the RELATIVE pairs become the edges bs_build takes into the band, the ordering and the packed all-reduce
void prior_store(BlockSys &bs, bool finalized, int32_t n, const lvba_prior *priors, std::vector<lvba_prior> &stored);
// FNV-1a over the stored priors' bytes, 62 bits (bs_ranks_agree negates it)
int64_t prior_hash(const std::vector<lvba_prior> &stored);

} // namespace lvba
