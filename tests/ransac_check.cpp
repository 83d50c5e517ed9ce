// ransac_check.cpp -- the tile-list arithmetic of csrc/ransac_device.h compiled for the host (tests/test_ransac_host.py): what
// ransac_run_hypotheses hands the hypothesis kernel as its grid.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/ransac_device.h"

using namespace lvba;

namespace {
struct Task { RansacSpan span; };
}

extern "C" {

// m [n_tasks] in; blk0, n_blk [n_tasks] in and out (a refusal leaves them as given).  build = 0: the count alone.
// build = 1: the list too; tiles [cap][2] = the first min(cap, n) tiles as (task, h0), last [2] = the last one.  Returns the number
// of blocks, -1 for a refusal (-2 if a refusal reserved memory, -3 if the list's length is not the count).
int64_t emul_plan(int64_t n_tasks, const int32_t *m, int32_t H, int32_t hb, int32_t need, int32_t build, int32_t *blk0, int32_t *n_blk,
                  int64_t cap, int32_t *tiles, int32_t *last)
{
    std::vector<Task> tasks((size_t)n_tasks);
    for (int64_t p = 0; p < n_tasks; ++p) tasks[p].span = RansacSpan{0, m[p], blk0[p], n_blk[p]};
    std::vector<RansacTile> list;
    const int64_t n = ransac_plan(tasks.data(), tasks.size(), H, hb, need, build ? &list : nullptr);
    for (int64_t p = 0; p < n_tasks; ++p) { blk0[p] = tasks[p].span.blk0; n_blk[p] = tasks[p].span.n_blk; }
    if (n < 0) return list.capacity() == 0 ? n : -2;
    if (!build) return n;
    if ((int64_t)list.size() != n) return -3;
    for (int64_t k = 0; k < n && k < cap; ++k) { tiles[2 * k] = list[k].task; tiles[2 * k + 1] = list[k].h0; }
    if (n > 0) { last[0] = list.back().task; last[1] = list.back().h0; }
    return n;
}

} // extern "C"
