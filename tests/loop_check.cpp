// loop_check.cpp -- csrc/loop_device.h compiled for the host (tests/test_loop_host.py): the candidate rule over all queries and
// submaps in plain loops, with the header's own arithmetic, comparisons and selection.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include "../global-lvba_amd/csrc/loop_device.h"

using namespace lvba;

extern "C" {

// pos [n][3]; out_* [capacity]; returns the true number of candidates
int64_t emul_candidates(int n, const double *pos, int submap_size, int min_gap, int max_per_frame, int query_stride, double radius,
                        int64_t capacity, int32_t *out_query, int32_t *out_submap, int32_t *out_ref, double *out_distance)
{
    const double radius2 = radius * radius;
    int64_t total = 0;
    const int n_sub = (int)(((int64_t)n + submap_size - 1) / submap_size);
    for (int j = 0; j < n; j += query_stride) {
        LoopBest top[LOOP_MAX_K];
        int32_t ref[LOOP_MAX_K];
        int kept = 0;
        for (int w = 0; w < n_sub; ++w) {
            const int f0 = w * submap_size, f1 = f0 + submap_size < n ? f0 + submap_size : n;
            if (!loop_gap_ok(j, f0, f1, min_gap)) continue;
            LoopBest b = loop_none();
            for (int f = f0; f < f1; ++f) {
                const double d2 = loop_d2(pos, j, f);
                if (loop_less(d2, f, b.d2, b.idx)) { b.d2 = d2; b.idx = f; }
            }
            if (!loop_in_radius(b.d2, radius2)) continue;
            loop_keep(top, ref, &kept, max_per_frame, b.d2, w, b.idx);
        }
        loop_sort_by_submap(top, ref, kept);
        for (int a = 0; a < kept; ++a, ++total) {
            if (total >= capacity) continue;
            out_query[total] = j; out_submap[total] = top[a].idx; out_ref[total] = ref[a]; out_distance[total] = sqrt(top[a].d2);
        }
    }
    return total;
}

int emul_gap_ok(int j, int f0, int f1, int min_gap) { return loop_gap_ok(j, f0, f1, min_gap) ? 1 : 0; }

} // extern "C"
