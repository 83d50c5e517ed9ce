// ransac_batch.h -- the device side of what the batched RANSAC stages have in common (verify.hip, resect.hip; DESIGN.md §10k "The
// skeleton"), on ransac_device.h' arithmetic.  A stage supplies a task struct with a RansacSpan member `span`, the length NM of
// its model in doubles, its hypothesis kernel (the sample, the solver, the scoring loop) between ransac_lane and
// ransac_block_best, its refine kernel, and two functors: inlier(task, task index, element) -> bool and emit(out, position,
// element), what one inlier writes into the call's list (WIDTH int32).  The grid of the hypothesis kernel is the list of (task,
// block of RANSAC_HB hypotheses) tiles of the whole call; a workgroup is one wavefront and a lane owns one hypothesis; its model
// reaches global memory only as the block's best, one record per block, and through the diagnostic calls.  No atomics, every
// choice an integer comparison: two calls give the same bytes, and so does a task alone or in a batch in any order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "segments.h"
#include "ransac_device.h"

namespace lvba {

constexpr int RANSAC_HB = 64;               // hypotheses per workgroup: one wavefront, a lane each
constexpr int64_t RANSAC_MAX_ELEMENTS = (int64_t)1 << 31;   // of all tasks of a call: the flags' prefix sum is 32 bits wide

template <int NM> struct RansacBest { int32_t count, h; double model[NM]; };   // count -1: no valid hypothesis

struct RansacLane { int32_t task, h; bool live; };   // live: h < H, the lane owns a hypothesis
__device__ __forceinline__ RansacLane ransac_lane(const RansacTile *__restrict__ tiles, int H)
{
    const RansacTile tl = tiles[blockIdx.x];
    const int32_t h = tl.h0 + (int32_t)threadIdx.x;
    return RansacLane{tl.task, h, h < H};
}

// count: the lane's inliers, -1 for an invalid hypothesis.  blk [n_tiles]; diag_model [H][NM], diag_count [H]: null, or every
// hypothesis of the one task (the diagnostic calls).
template <int NM>
__device__ __forceinline__ void ransac_block_best(const RansacLane &ln, int32_t count, const double *model, RansacBest<NM> *__restrict__ blk,
                                                  double *__restrict__ diag_model, int32_t *__restrict__ diag_count)
{
    if (diag_model && ln.live) {
#pragma unroll
        for (int k = 0; k < NM; ++k) diag_model[NM * (int64_t)ln.h + k] = model[k];
        diag_count[ln.h] = count;
    }
    const int64_t own = ln.live ? ransac_rank(count, ln.h) : (int64_t)-1;
    int64_t top = own;
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const int64_t o = __shfl_xor(top, w, 64);
        top = o > top ? o : top;
    }
    if (ln.live && own == top) { // one lane: h is part of the rank
        RansacBest<NM> &b = blk[blockIdx.x];
        b.count = count; b.h = ln.h;
#pragma unroll
        for (int k = 0; k < NM; ++k) b.model[k] = model[k];
    }
}

// The hypotheses of every task with at least `need` elements, one grid: launch(n_tiles, tiles) starts the stage's kernel on s.
// blk0 / n_blk of the tasks are set here, before they go up.  d_blk: the block records.
template <int NM, class Task, class Launch>
int32_t ransac_run_hypotheses(hipStream_t s, std::vector<Task> &tasks, int32_t H, int32_t need, DevArr<Task> &d_tasks,
                              DevArr<RansacBest<NM>> &d_blk, const Launch &launch)
{
    std::vector<RansacTile> tiles;
    if (ransac_plan(tasks.data(), tasks.size(), H, RANSAC_HB, need, &tiles) < 0)
        return lvba_fail(LVBA_ERR_UNSUPPORTED, "more than 2^30 hypothesis blocks in one call");
    HIPCHK(d_tasks.alloc_upload(tasks)); HIPCHK(d_blk.alloc(tiles.size()));
    if (tiles.empty()) return LVBA_OK;
    DevArr<RansacTile> d_tiles(s);
    HIPCHK(d_tiles.alloc_upload(tiles));
    launch((unsigned)tiles.size(), d_tiles);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s)); // the tile list goes with this scope
    return LVBA_OK;
}

// res [n_tasks]: the task's best block record; count -1, h -1 and a zero model where it has none
template <int NM, class Task>
__global__ __launch_bounds__(256) void ransac_pick_kernel(int n_tasks, const Task *__restrict__ tasks, const RansacBest<NM> *__restrict__ blk,
                                                          RansacBest<NM> *__restrict__ res)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_tasks) return;
    const RansacBest<NM> *mine = blk + tasks[p].span.blk0;
    const int32_t win = ransac_winner(tasks[p].span.n_blk, [=](int32_t k) { return mine[k].count; }, [=](int32_t k) { return mine[k].h; });
    RansacBest<NM> b;
    b.count = -1; b.h = -1;
#pragma unroll
    for (int k = 0; k < NM; ++k) b.model[k] = 0.0;
    if (win >= 0) b = mine[win];
    res[p] = b;
}

// flag [n + 1] (the last is 0): element i of the call is an inlier of its task's final model and the task is OK
template <class Task, class Inlier>
__global__ __launch_bounds__(256) void ransac_mask_kernel(int64_t n, int n_tasks, const Task *__restrict__ tasks,
                                                          const int32_t *__restrict__ status, Inlier inlier, uint32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { flag[i] = 0; return; }
    const int j = segment_of([=](int k) { return tasks[k].span.off; }, n_tasks, i);
    flag[i] = status[j] == RANSAC_OK && inlier(tasks[j], j, i) ? 1u : 0u;
}

// out [n_out][Emit::WIDTH]: what the inliers emit, in (task, original order); off [n_tasks + 1]
template <class Task, class Emit>
__global__ __launch_bounds__(256) void ransac_write_kernel(int64_t n, int n_tasks, const Task *__restrict__ tasks,
                                                           const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl, int64_t n_out,
                                                           Emit emit, int32_t *__restrict__ out, int64_t *__restrict__ off)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_tasks) off[i] = excl[tasks[i].span.off];
    if (i == n_tasks) off[i] = excl[n];
    if (i >= n || !flag[i]) return;
    const int64_t pos = excl[i];
    if (pos >= n_out) return;
    emit(out, pos, i);
}

// The inlier lists of a call of n_tasks >= 1 tasks over `total` elements, from the tasks' final models (inside `inlier`) and
// statuses: inlier_off [n_tasks + 1] always, the first min(found, capacity) entries of `inliers`.  total < RANSAC_MAX_ELEMENTS.
template <class Task, class Inlier, class Emit>
int32_t ransac_inlier_lists(hipStream_t s, int64_t total, int n_tasks, const Task *d_tasks, const int32_t *d_status, const Inlier &inlier,
                            const Emit &emit, int64_t capacity, int64_t *inlier_off, int32_t *inliers)
{
    DevArr<uint32_t> d_flag(s), d_excl(s); DevArr<int64_t> d_off(s); DevArr<int32_t> d_out(s);
    HIPCHK(d_flag.alloc((size_t)total + 1)); HIPCHK(d_excl.alloc((size_t)total + 1)); HIPCHK(d_off.alloc((size_t)n_tasks + 1));
    ransac_mask_kernel<<<grid_for(total + 1, 256), 256, 0, s>>>(total, n_tasks, d_tasks, d_status, inlier, d_flag);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, d_flag, d_excl, (size_t)total + 1));
    uint32_t found = 0;
    HIPCHK(copy_d2h(&found, d_excl + total, d_excl.bytes(1)));
    const int64_t n_out = std::min<int64_t>(found, capacity);
    HIPCHK(d_out.alloc(Emit::WIDTH * (size_t)n_out));
    ransac_write_kernel<<<grid_for(std::max<int64_t>(total, n_tasks + 1), 256), 256, 0, s>>>(
        total, n_tasks, d_tasks, d_flag, d_excl, n_out, emit, d_out, d_off);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(d_off.download(inlier_off, (size_t)n_tasks + 1));
    if (n_out > 0) HIPCHK(d_out.download(inliers, Emit::WIDTH * (size_t)n_out));
    return LVBA_OK;
}

// mask [task.span.m], span.m >= 1: element i of the one task is an inlier of the model inside `inlier`
template <class Task, class Inlier>
int32_t ransac_score_mask(hipStream_t s, const Task &task, const Inlier &inlier, uint8_t *mask)
{
    const size_t n = (size_t)task.span.m;
    const int32_t ok = RANSAC_OK;
    DevArr<Task> d_tasks(s); DevArr<int32_t> d_st(s); DevArr<uint32_t> d_flag(s);
    HIPCHK(d_tasks.alloc(1)); HIPCHK(d_st.alloc(1)); HIPCHK(d_flag.alloc(n + 1)); HIPCHK(d_tasks.upload(&task, 1));
    HIPCHK(d_st.upload(&ok, 1));
    ransac_mask_kernel<Task><<<grid_for((int64_t)n + 1, 256), 256, 0, s>>>((int64_t)n, 1, d_tasks, d_st, inlier,
                                                                    d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    std::vector<uint32_t> flag(n);
    HIPCHK(d_flag.download(flag.data(), n));
    for (size_t i = 0; i < n; ++i) mask[i] = flag[i] ? 1 : 0;
    return LVBA_OK;
}

} // namespace lvba
