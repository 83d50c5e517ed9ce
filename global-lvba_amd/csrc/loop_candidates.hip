// loop_candidates.hip -- loop-closure candidate search: which frame revisits which submap, from the frames' positions alone
// (lvba_loop_candidates; the rule is in include/lvba_hip.h, its scalar arithmetic in loop_device.h, also compiled for the host by
// the tests).
//
// Device design, two launches around one scan:
//   loop_search_kernel   one wavefront per query frame j, four to a workgroup.  The wavefront walks the submaps in index order; a
//                        submap that fails the gap clause costs two scalar compares.  Otherwise the lanes stride over the submap's
//                        frames, each keeps its smallest (d2, f) pair; if no lane is inside the radius the submap is done (one
//                        ballot), else the pairs are reduced in a fixed order -- the DPP tree of wave_ops.h
//                        (wave_fold_to_lane63 with MinPairStep) on the pair, compared lexicographically -- and lane 0 files the result among the
//                        query's max_per_frame best in LDS.  At the end lane 0 puts them in submap order into the query's slot of a
//                        staging array and writes their number.
//   scan_excl            where every query's entries begin; the last element is the total.
//   loop_write_kernel    one lane per query copies its entries to their place, up to `capacity` (loop_device.h; shared with
//                        place.hip).
// No atomics anywhere, every minimum in a fixed order: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "loop_device.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int LOOP_BLOCK = 256; // four wavefronts, a query each

// count [nq], stage [nq][max_per_frame]
__global__ __launch_bounds__(LOOP_BLOCK) void loop_search_kernel(int n, int nq, const double *__restrict__ pos, const LoopParams o,
                                                                 int64_t *__restrict__ count, lvba_loop_candidate *__restrict__ stage)
{
    __shared__ LoopBest top[LOOP_BLOCK / 64][LOOP_MAX_K];
    __shared__ int32_t ref[LOOP_BLOCK / 64][LOOP_MAX_K];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * (LOOP_BLOCK / 64) + wv;
    if (q >= nq) return; // (the whole wavefront; the workgroup never synchronises)
    const int j = (int)((int64_t)q * o.query_stride);
    const int64_t S = o.submap_size;
    const int n_sub = (int)((n + S - 1) / S);
    int kept = 0; // lane 0's
    for (int w = 0; w < n_sub; ++w) {
        const int f0 = (int)(w * S), f1 = (int)(w * S + S < n ? w * S + S : n);
        if (!loop_gap_ok(j, f0, f1, o.min_gap)) continue;
        LoopBest b = loop_none();
        for (int f = f0 + lane; f < f1; f += 64) {
            const double d2 = loop_d2(pos, j, f);
            if (loop_less(d2, f, b.d2, b.idx)) { b.d2 = d2; b.idx = f; }
        }
        if (!__any(loop_in_radius(b.d2, o.radius2) ? 1 : 0)) continue;
        b = wave_fold_to_lane63<MinPairStep<LoopBest>>(b);
        const double d2 = readlane_f64(b.d2, 63);
        const int f = __builtin_amdgcn_readlane(b.idx, 63);
        if (lane == 0) loop_keep(top[wv], ref[wv], &kept, o.max_per_frame, d2, w, f);
    }
    if (lane != 0) return;
    loop_sort_by_submap(top[wv], ref[wv], kept);
    count[q] = kept;
    for (int a = 0; a < kept; ++a) {
        lvba_loop_candidate c;
        c.query = j; c.submap = top[wv][a].idx; c.ref = ref[wv][a]; c.pad = 0;
        c.distance = sqrt(top[wv][a].d2);
        stage[(int64_t)q * o.max_per_frame + a] = c;
    }
}

} // namespace

extern "C" void lvba_loop_default_opts(lvba_loop_opts *o)
{
    if (!o) return;
    *o = lvba_loop_opts{};
    o->submap_size = 10;
    o->min_gap = 50;
    o->max_per_frame = 2;
    o->query_stride = 1;
    o->radius = 5.0;
}

extern "C" int32_t lvba_loop_candidates(int32_t device, int32_t n_frames, const double *poses, const lvba_loop_opts *opts, int64_t capacity,
                                        lvba_loop_candidate *out, int64_t *count)
{
    if (!count || n_frames < 0 || capacity < 0 || (n_frames > 0 && !poses) || (capacity > 0 && !out))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_frames < 0 or capacity < 0");
    *count = 0;
    lvba_loop_opts o;
    lvba_loop_default_opts(&o);
    if (opts) o = *opts;
    if (o.submap_size < 1 || o.min_gap < 0 || o.max_per_frame < 1 || o.max_per_frame > LOOP_MAX_K || o.query_stride < 1 ||
        !(o.radius > 0.0) || !std::isfinite(o.radius))
        return lvba_fail(LVBA_ERR_ARG, "options: submap_size %d (>= 1), min_gap %d (>= 0), max_per_frame %d (1 .. %d), query_stride %d (>= 1), "
                         "radius %g (finite and > 0)", o.submap_size, o.min_gap, o.max_per_frame, LOOP_MAX_K, o.query_stride, o.radius);
    const int n = n_frames;
    std::vector<double> pos(3 * (size_t)n);
    for (int f = 0; f < n; ++f)
        for (int a = 0; a < 12; ++a) {
            const double v = poses[12 * (size_t)f + a];
            if (!std::isfinite(v)) return lvba_fail(LVBA_ERR_ARG, "frame %d: non-finite pose", f);
            if (a >= 9) pos[3 * (size_t)f + (a - 9)] = v;
        }
    if (n == 0) return LVBA_OK;
    LoopParams par;
    par.submap_size = o.submap_size; par.min_gap = o.min_gap; par.max_per_frame = o.max_per_frame; par.query_stride = o.query_stride;
    par.radius2 = o.radius * o.radius;
    const int nq = (int)(((int64_t)n + o.query_stride - 1) / o.query_stride);
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    DevArr<double> d_pos(s); DevArr<int64_t> d_count(s), d_first(s); DevArr<lvba_loop_candidate> d_stage(s), d_out(s);
    HIPCHK(d_pos.alloc(3 * (size_t)n)); HIPCHK(d_count.alloc((size_t)nq + 1)); HIPCHK(d_first.alloc((size_t)nq + 1));
    HIPCHK(d_stage.alloc((size_t)nq * (size_t)o.max_per_frame)); HIPCHK(d_pos.upload(pos.data(), 3 * (size_t)n));
    HIPCHK(d_count.zero_async(1, nq));
    loop_search_kernel<<<grid_for(nq, LOOP_BLOCK / 64), LOOP_BLOCK, 0, s>>>(n, nq, d_pos, par, d_count,
                                                                           d_stage);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<int64_t>(s, d_count, d_first, (size_t)nq + 1));
    int64_t total = 0;
    HIPCHK(copy_d2h(&total, d_first + nq, d_first.bytes(1)));
    *count = total;
    const int64_t n_out = std::min(total, capacity);
    if (n_out == 0) return LVBA_OK;
    HIPCHK(d_out.alloc((size_t)n_out));
    loop_write_kernel<lvba_loop_candidate><<<grid_for(nq, 256), 256, 0, s>>>(nq, o.max_per_frame, d_count, d_first,
                                                        d_stage, n_out, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(d_out.download(out, (size_t)n_out));
    return LVBA_OK;
}
