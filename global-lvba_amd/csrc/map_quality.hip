// map_quality.hip -- map quality without ground truth, on the device: the mean map entropy and mean plane variance of
// Razlaw et al. 2015 over the aggregated LiDAR cloud, with the per-point entropy, plane variance, normal and neighbour count.
// The per-point rules are map_quality_device.h (also compiled for the host by the tests); the definitions are in
// include/lvba_hip.h and DESIGN.md §10b.
//
// Device design: a fixed-radius neighbourhood reduction over a uniform grid of cells with an edge just above the radius.
//   1. key      one lane per point: the cell key (pack_key's 3 x 21 bits), non-finite points take a key above every cell; the
//               range of the components is reduced on the way (voxel_internal.h) and the keys are re-packed on the bits that vary
//   2. sort     one stable radix sort of (key, point index); the points are gathered into sorted order as 16-byte records
//               (x, y, z, index); run heads give the table of unique cell keys and their first positions; the queries
//               (index % stride == 0) are listed in sorted order
//   3. reduce   one wavefront per 64 consecutive queries of that list, lane = query.  Keys order by (x, y, z), so the cells
//               (x, y, z-1 .. z+1) are one contiguous range of the sorted points and a query's 27 cells are 9 ranges.  The lanes
//               of a wavefront that share a cell COLUMN (x, y) form a segment (sorted order makes it a run of lanes) and share
//               the 9 ranges (x+-1, y+-1, zmin-1 .. zmax+1), found by two binary searches each in the unique-key table by
//               lanes 0 .. 8.  A dense map has one or two segments per wavefront, a sparse one many short ones: no table of
//               work items, and no lane idles because its cell holds few queries.  The ranges are walked in tiles of 64
//               candidates: one coalesced 16-byte load per lane, widened once to double into LDS; every lane then reads the same
//               candidate (an LDS broadcast), tests d2 <= r2 and accumulates the count and 9 moments in registers.  The candidate
//               order is the sorted order, whatever the segment: the per-query sums need no cross-lane reduction and no
//               atomics, and do not depend on the stride or on which other queries share the wavefront.
//               Then covariance, eigen-pair, entropy (map_quality_device.h), written at the query's index, and the five grid
//               sums in the fixed order of prior_grid_sum (prior_device.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "colorize_device.h"
#include "prior_device.h"
#include "map_quality_device.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr uint64_t MAPQ_NO_CELL = ~(uint64_t)0; // key of a non-finite point: above every cell key
constexpr int MAPQ_TILE = 64;

// 1. cell keys and their range.  Every lane of every wavefront reaches key_range_update.
__global__ __launch_bounds__(256) void mapq_key_kernel(int64_t n, const float *__restrict__ world, double edge, uint64_t *__restrict__ key,
                                                       int *__restrict__ partial, int *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kb[3] = {0, 0, 0};
    bool valid = false;
    if (i < n) {
        const float w[3] = {world[3 * i], world[3 * i + 1], world[3 * i + 2]};
        uint64_t k = MAPQ_NO_CELL;
        if (mapq_finite(w)) {
            int64_t c[3];
            if (mapq_cell_of(w, edge, c)) {
                valid = true;
                k = pack_key(c);
                for (int j = 0; j < 3; ++j) kb[j] = (int)(c[j] + KEY_BIAS);
            } else {
                atomicOr(err, 1);
            }
        }
        key[i] = k;
    }
    key_range_update(partial, kb, valid);
}

__global__ void mapq_compress_kernel(int64_t n, const uint64_t *__restrict__ key, const KeyPack kp, uint64_t *__restrict__ ckey,
                                     uint32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i];
    ckey[i] = k == MAPQ_NO_CELL ? (uint64_t)1 << kp.total : key_compress<uint64_t>(k, kp);
    idx[i] = (uint32_t)i;
}

// 2. sorted records, run heads, query flags
__global__ void mapq_gather_kernel(int64_t n, const uint64_t *__restrict__ ckey_s, const uint32_t *__restrict__ idx_s,
                                   const float *__restrict__ world, uint32_t stride, float4 *__restrict__ rec, uint32_t *__restrict__ head,
                                   uint32_t *__restrict__ qflag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = idx_s[i];
    rec[i] = make_float4(world[3 * (int64_t)p], world[3 * (int64_t)p + 1], world[3 * (int64_t)p + 2], __uint_as_float(p));
    head[i] = (i == 0 || ckey_s[i] != ckey_s[i - 1]) ? 1u : 0u;
    qflag[i] = p % stride == 0 ? 1u : 0u;
}
// ukey [n_cells], ustart [n_cells + 1] (ustart[n_cells] = n), qlist [n_queries] = the sorted positions of the queries
__global__ void mapq_table_kernel(int64_t n, const uint64_t *__restrict__ ckey_s, const uint32_t *__restrict__ head,
                                  const uint32_t *__restrict__ head_x, const uint32_t *__restrict__ qflag, const uint32_t *__restrict__ q_x,
                                  const KeyPack kp, int64_t n_cells, uint64_t *__restrict__ ukey, uint32_t *__restrict__ ustart,
                                  uint32_t *__restrict__ qlist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (head[i]) {
        const uint64_t c = ckey_s[i];
        ukey[head_x[i]] = c == (uint64_t)1 << kp.total ? MAPQ_NO_CELL : key_expand<uint64_t>(c, kp);
        ustart[head_x[i]] = (uint32_t)i;
    }
    if (qflag[i]) qlist[q_x[i]] = (uint32_t)i;
    if (i == 0) ustart[n_cells] = (uint32_t)n;
}

// first index in [0, n) with a[index] >= v (upper: > v)
__device__ __forceinline__ int64_t mapq_bound(const uint64_t *__restrict__ a, int64_t n, uint64_t v, bool upper)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t x = a[mid];
        if (upper ? x <= v : x < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// 3. the reduction: 64 lanes = 64 consecutive queries of qlist.  part [gridDim.x][5], sums [5] = entropy, plane_var, valid
// queries, neighbours, queries with a finite point.
__global__ __launch_bounds__(64) void mapq_reduce_kernel(int64_t nq, const uint32_t *__restrict__ qlist, const float4 *__restrict__ rec,
                                                         const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ ustart,
                                                         int64_t n_cells, double edge, double r2, int min_neighbors, uint32_t stride,
                                                         double *__restrict__ entropy, double *__restrict__ plane_var,
                                                         float *__restrict__ normal, int32_t *__restrict__ count,
                                                         double *__restrict__ part, unsigned *__restrict__ ticket, double *__restrict__ sums)
{
    __shared__ double tile[MAPQ_TILE][4];
    const int lane = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const bool active = q < nq;
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) me = rec[qlist[q]];
    const float wf[3] = {me.x, me.y, me.z};
    const double wq[3] = {(double)me.x, (double)me.y, (double)me.z};
    const bool fin = active && mapq_finite(wf);
    int64_t c[3] = {0, 0, 0};
    if (fin) mapq_cell_of(wf, edge, c); // in range: the key kernel checked every finite point
    const int bx = (int)c[0] + KEY_BIAS, by = (int)c[1] + KEY_BIAS, bz = (int)c[2] + KEY_BIAS; // biased
    MapqAcc acc;
    mapq_clear(acc);
    bool todo = fin;
    for (;;) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int leader = __ffsll(m) - 1;
        const int lx = __shfl(bx, leader), ly = __shfl(by, leader);
        const bool mine = todo && bx == lx && by == ly;
        const unsigned long long mm = __ballot(mine);
        const int z1 = __shfl(bz, leader), z2 = __shfl(bz, 63 - __clzll(mm)); // sorted: the segment's first and last cell
        uint32_t r_begin = 0, r_end = 0;
        if (lane < 9) {
            const uint64_t X = (uint64_t)(lx + lane / 3 - 1), Y = (uint64_t)(ly + lane % 3 - 1);
            const uint64_t base = (X << 42) | (Y << 21);
            r_begin = ustart[mapq_bound(ukey, n_cells, base | (uint64_t)(z1 - 1), false)];
            r_end = ustart[mapq_bound(ukey, n_cells, base | (uint64_t)(z2 + 1), true)];
        }
        for (int r = 0; r < 9; ++r) {
            const int64_t b = __shfl(r_begin, r), e = __shfl(r_end, r);
            for (int64_t t0 = b; t0 < e; t0 += MAPQ_TILE) {
                const int cnt = (int)std::min<int64_t>(MAPQ_TILE, e - t0);
                __syncthreads();
                if (lane < cnt) {
                    const float4 p = rec[t0 + lane];
                    tile[lane][0] = (double)p.x; tile[lane][1] = (double)p.y; tile[lane][2] = (double)p.z;
                }
                __syncthreads();
                if (mine) {
#pragma unroll 4
                    for (int j = 0; j < cnt; ++j) mapq_visit(acc, wq, tile[j][0], tile[j][1], tile[j][2], r2);
                }
            }
        }
        todo = todo && !mine;
    }
    MapqOut o;
    mapq_finish(acc, min_neighbors, o);
    if (active) {
        const int64_t k = (int64_t)(__float_as_uint(me.w) / stride);
        entropy[k] = o.entropy;
        plane_var[k] = o.plane_var;
        normal[3 * k] = o.normal[0]; normal[3 * k + 1] = o.normal[1]; normal[3 * k + 2] = o.normal[2];
        count[k] = acc.n;
    }
    const double v[5] = {o.valid ? o.entropy : 0.0, o.valid ? o.plane_var : 0.0, o.valid ? 1.0 : 0.0, fin ? (double)acc.n : 0.0,
                         fin ? 1.0 : 0.0};
    double *const out[5] = {sums, sums + 1, sums + 2, sums + 3, sums + 4};
    prior_grid_sum<5>(v, part, ticket, out, false);
}

int32_t check_opts(const lvba_mapq_opts *opts, lvba_mapq_opts &o)
{
    lvba_mapq_default_opts(&o);
    if (opts) o = *opts;
    if (!(o.radius > 0.0) || !std::isfinite(o.radius) || o.min_neighbors < 4 || o.query_stride < 1)
        return lvba_fail(LVBA_ERR_ARG, "options: radius %g (> 0), min_neighbors %d (>= 4), query_stride %d (>= 1)", o.radius,
                         o.min_neighbors, o.query_stride);
    return LVBA_OK;
}

// bytes the run needs for n points on top of the world points themselves (keys, sorted copies, records, flags, scans, the
// sort's scratch) and per query (list, outputs)
double mapq_bytes(int64_t n, int64_t nq) { return 108.0 * (double)n + 40.0 * (double)nq + (double)(1 << 20); }

int32_t fits(int64_t n, int64_t nq, double extra)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double have = (double)free_b + (double)DevicePool::get().cached_bytes();
    if (mapq_bytes(n, nq) + extra > 0.9 * have)
        return lvba_fail(LVBA_ERR_NOMEM, "map quality: %lld points need %.0f MB of device memory, %.0f MB are free", (long long)n,
                         (mapq_bytes(n, nq) + extra) / 1048576.0, have / 1048576.0);
    return LVBA_OK;
}

// the metrics of n world points on the device (stream s, the current device); ms[0] is the caller's
int32_t mapq_run(hipStream_t s, const float *d_world, int64_t n, const lvba_mapq_opts &o, lvba_mapq_summary *sum, double *entropy,
                 double *plane_var, float *normal, int32_t *count, EventTimer<4> &ev)
{
    const int64_t stride = o.query_stride;
    const int64_t nq = (n + stride - 1) / stride;
    sum->n_points = n; sum->n_queries = nq; sum->n_valid = 0;
    sum->mme = sum->mpv = sum->mean_neighbors = NAN;
    if (n == 0) return LVBA_OK;
    const double edge = mapq_cell_edge(o.radius), r2 = o.radius * o.radius;
    // 1. keys
    DevArr<uint64_t> key(s); DevArr<int> partial(s), small(s); DevArr<uint64_t> ckey(s); DevArr<uint32_t> idx(s);
    DevArr<uint64_t> ckey_s(s); DevArr<uint32_t> idx_s(s);
    const int64_t slots = key_range_slots(n, 256);
    HIPCHK(key.alloc((size_t)n)); HIPCHK(partial.alloc(6 * (size_t)slots)); HIPCHK(small.alloc(16));
    HIPCHK(small.zero_async(16)); // rng[6], err, ticket
    int *d_rng = small, *d_err = d_rng + 6;
    unsigned *d_ticket = (unsigned *)(d_rng + 7);
    mapq_key_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, d_world, edge, key, partial, d_err);
    HIPCHK(hipGetLastError());
    key_range_reduce_kernel<<<key_range_reduce_grid(slots), 256, 0, s>>>(slots, partial, d_rng);
    HIPCHK(hipGetLastError());
    int host[7] = {0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(host, d_rng, sizeof(host), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (host[6])
        return lvba_fail(LVBA_ERR_ARG, "map quality: a point lies 2^20 - 1 or more cells of %g m from the origin", edge);
    const KeyPack kp = key_pack_of(host);
    // 2. sort, records, tables
    HIPCHK(ckey.alloc((size_t)n)); HIPCHK(idx.alloc((size_t)n)); HIPCHK(ckey_s.alloc((size_t)n)); HIPCHK(idx_s.alloc((size_t)n));
    mapq_compress_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, key, kp, ckey, idx);
    HIPCHK(hipGetLastError());
    TRY(sort_pairs<uint64_t>(s, ckey, ckey_s, idx, idx_s, (size_t)n, (unsigned)kp.total + 1));
    DevArr<float4> rec(s); DevArr<uint32_t> head(s), head_x(s), qflag(s), q_x(s); DevArr<uint64_t> ukey(s);
    DevArr<uint32_t> ustart(s), qlist(s);
    HIPCHK(rec.alloc((size_t)n)); HIPCHK(head.alloc((size_t)n)); HIPCHK(head_x.alloc((size_t)n));
    HIPCHK(qflag.alloc((size_t)n)); HIPCHK(q_x.alloc((size_t)n));
    mapq_gather_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, ckey_s, idx_s, d_world, (uint32_t)stride, rec, head, qflag);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<uint32_t>(s, qflag, q_x, (size_t)n));
    int64_t n_cells = 0;
    TRY(count_flags(s, head, head_x, (size_t)n, &n_cells));
    HIPCHK(ukey.alloc((size_t)n_cells)); HIPCHK(ustart.alloc((size_t)(n_cells + 1))); HIPCHK(qlist.alloc((size_t)nq));
    mapq_table_kernel<<<grid_for(n, 256), 256, 0, s>>>(n, ckey_s, head, head_x, qflag, q_x, kp, n_cells, ukey, ustart, qlist);
    HIPCHK(hipGetLastError());
    ev.rec(2, s);
    // 3. reduction
    const unsigned grid = grid_for(nq, 64);
    DevArr<double> d_ent(s), d_pv(s); DevArr<float> d_nrm(s); DevArr<int32_t> d_cnt(s); DevArr<double> part(s), sums(s);
    HIPCHK(d_ent.alloc((size_t)nq)); HIPCHK(d_pv.alloc((size_t)nq)); HIPCHK(d_nrm.alloc(3 * (size_t)nq));
    HIPCHK(d_cnt.alloc((size_t)nq)); HIPCHK(part.alloc(5 * (size_t)grid)); HIPCHK(sums.alloc(5));
    mapq_reduce_kernel<<<grid, 64, 0, s>>>(nq, qlist, rec, ukey, ustart, n_cells, edge, r2, o.min_neighbors, (uint32_t)stride,
                                           d_ent, d_pv, d_nrm, d_cnt, part, d_ticket, sums);
    HIPCHK(hipGetLastError());
    ev.rec(3, s);
    double h_sums[5] = {0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h_sums, sums, sizeof(h_sums), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    sum->ms[1] = ev.ms(1, 2);
    sum->ms[2] = ev.ms(2, 3);
    // 4. download
    const double t0 = now_ms();
    if (entropy) HIPCHK(d_ent.download(entropy, (size_t)nq));
    if (plane_var) HIPCHK(d_pv.download(plane_var, (size_t)nq));
    if (normal) HIPCHK(d_nrm.download(normal, 3 * (size_t)nq));
    if (count) HIPCHK(d_cnt.download(count, (size_t)nq));
    sum->ms[3] = now_ms() - t0;
    sum->n_valid = (int64_t)h_sums[2];
    if (h_sums[2] > 0.0) { sum->mme = h_sums[0] / h_sums[2]; sum->mpv = h_sums[1] / h_sums[2]; }
    if (h_sums[4] > 0.0) sum->mean_neighbors = h_sums[3] / h_sums[4];
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_mapq_default_opts(lvba_mapq_opts *o)
{
    if (!o) return;
    o->radius = 0.3;
    o->min_neighbors = 8;
    o->query_stride = 1;
}

extern "C" int32_t lvba_mapq_scans(lvba_scans_t sc, const double *scan_poses, int32_t frame_begin, int32_t n_frames,
                                   const lvba_mapq_opts *opts, lvba_mapq_summary *summary, double *entropy, double *plane_var,
                                   float *normal, int32_t *count)
{
    if (!sc || !scan_poses || !summary) return lvba_fail(LVBA_ERR_ARG, "null argument");
    lvba_mapq_opts o;
    TRY(check_opts(opts, o));
    if (frame_begin < 0 || n_frames < 1 || (int64_t)frame_begin + n_frames > sc->n_frames)
        return lvba_fail(LVBA_ERR_ARG, "frames [%d, %d + %d) of %d", frame_begin, frame_begin, n_frames, sc->n_frames);
    for (int64_t i = 0; i < 12 * (int64_t)n_frames; ++i)
        if (!std::isfinite(scan_poses[i])) return lvba_fail(LVBA_ERR_ARG, "non-finite scan pose");
    *summary = lvba_mapq_summary{};
    const int64_t P = sc->frame_off[frame_begin + n_frames] - sc->frame_off[frame_begin];
    if (P >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_ARG, "%lld points (at most 2^32 - 1)", (long long)P);
    HIPCHK(hipSetDevice(sc->device));
    TRY(fits(P, (P + o.query_stride - 1) / o.query_stride, 12.0 * (double)P));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<4> ev;
    DevArr<float> world(s); DevArr<double> d_poses(s);
    HIPCHK(world.alloc(3 * (size_t)std::max<int64_t>(P, 1))); HIPCHK(d_poses.alloc(12 * (size_t)n_frames));
    HIPCHK(hipMemcpyAsync(d_poses, scan_poses, d_poses.bytes(12 * (size_t)n_frames), hipMemcpyHostToDevice, s));
    ev.rec(0, s);
    if (P > 0) {
        col_world_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, sc->d_pts + 3 * sc->frame_off[frame_begin],
                                                          sc->d_frame_off + frame_begin, n_frames, d_poses, 0.0, 0, world, nullptr);
        HIPCHK(hipGetLastError());
    }
    ev.rec(1, s);
    const int32_t rc = mapq_run(s, world, P, o, summary, entropy, plane_var, normal, count, ev);
    HIPCHK(hipStreamSynchronize(s)); // scan_poses was read by now
    if (rc == LVBA_OK) summary->ms[0] = ev.ms(0, 1);
    return rc;
}

extern "C" int32_t lvba_mapq_points(int32_t device, int64_t n, const float *xyz, const lvba_mapq_opts *opts, lvba_mapq_summary *summary,
                                    double *entropy, double *plane_var, float *normal, int32_t *count)
{
    if (!summary || n < 0 || (n > 0 && !xyz)) return lvba_fail(LVBA_ERR_ARG, "null argument or n < 0");
    lvba_mapq_opts o;
    TRY(check_opts(opts, o));
    if (n >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_ARG, "%lld points (at most 2^32 - 1)", (long long)n);
    *summary = lvba_mapq_summary{};
    HIPCHK(hipSetDevice(device));
    TRY(fits(n, (n + o.query_stride - 1) / o.query_stride, 12.0 * (double)n));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    EventTimer<4> ev;
    DevArr<float> world(s);
    HIPCHK(world.alloc(3 * (size_t)std::max<int64_t>(n, 1)));
    const double t0 = now_ms();
    if (n > 0) HIPCHK(world.upload(xyz, 3 * (size_t)n));
    const double up = now_ms() - t0;
    ev.rec(1, s);
    const int32_t rc = mapq_run(s, world, n, o, summary, entropy, plane_var, normal, count, ev);
    if (rc == LVBA_OK) summary->ms[0] = up;
    return rc;
}
