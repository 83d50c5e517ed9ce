// place.hip -- scan-descriptor place recognition: which frame revisits which submap, from the clouds alone (lvba_place_*; the
// rule is in include/lvba_hip.h, its scalar arithmetic in place_device.h, also compiled for the host by the tests; DESIGN.md
// §10e).
//
// Device design:
//   place_describe_kernel  a few workgroups per frame stream the frame's points (12 B each, lane-consecutive).  The Nr x Ns image
//                          lives in LDS as the bits of non-negative floats and takes an integer max per point; at the end a frame
//                          with one workgroup stores its cells, a frame with several merges them with a global integer max.  A
//                          maximum does not depend on the order: the same bytes every call.
//   place_finish_kernel    one workgroup per frame: the ring key (a thread per ring), the fp64 normalised columns in ring-major
//                          layout and the mask of non-empty columns (a thread per sector, the mask by ballot).
//   place_key_kernel       one wavefront per query, four to a workgroup.  The lanes stride over a tile of frames and put the fp32
//                          key distance of each (inf: the frame's submap fails the gap clause) into LDS once; then up to K rounds
//                          of the lexicographic wave-wide minimum "greater than the previous pick" (wave_fold_to_lane63 with
//                          MinPairStep) walk the tile in ascending order and lane 0 files each pick among the K best so far --
//                          K insertions per tile, not one per frame -- until a pick no longer improves the list.
//   place_shift_kernel     one wavefront per (query, picked frame): both U in LDS, lane = shift (the lanes loop for Ns > 64), every
//                          lane walks (j, ring) in order -- U_c a broadcast, U_q lane-consecutive --, then one lexicographic
//                          (dist, shift) minimum across the wavefront.
//   place_select_kernel    one wavefront per query, lane = pick: the per-submap ref, the max_distance gate, the max_per_frame cut
//                          and the submap order as three counting passes over the K picks in LDS.
//   scan_excl, loop_write_kernel   as lvba_loop_candidates.
// No floating-point atomics, every sum and every minimum in a fixed order: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "place_device.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int DESC_BLOCK = 256;        // place_describe_kernel
constexpr int DESC_PART_POINTS = 16384; // points per workgroup a frame is cut into, up to DESC_MAX_PARTS workgroups
constexpr int DESC_MAX_PARTS = 16;
constexpr int FIN_BLOCK = PLACE_MAX_SECTORS; // a thread per sector
constexpr int KEY_BLOCK = 256;         // four wavefronts, a query each
constexpr int KEY_TILE = 1024;         // frames whose key distance a wavefront holds in LDS

// desc [n][Nr * Ns], zeroed by the caller when parts > 1; grid (parts, n)
__global__ __launch_bounds__(DESC_BLOCK) void place_describe_kernel(const float *__restrict__ pts, const int64_t *__restrict__ frame_off,
                                                                    int frame_begin, const PlaceParams o, float *__restrict__ desc)
{
    extern __shared__ uint32_t img[];
    const int cells = o.n_rings * o.n_sectors;
    for (int c = threadIdx.x; c < cells; c += DESC_BLOCK) img[c] = 0u;
    __syncthreads();
    const int f = blockIdx.y, parts = gridDim.x;
    const int64_t p1 = frame_off[frame_begin + f + 1];
    for (int64_t i = frame_off[frame_begin + f] + (int64_t)blockIdx.x * DESC_BLOCK + threadIdx.x; i < p1; i += (int64_t)parts * DESC_BLOCK) {
        float h;
        const int c = place_bin(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], o, &h);
        if (c >= 0) atomicMax(&img[c], __float_as_uint(h)); // h > 0: the bits order as the values
    }
    __syncthreads();
    uint32_t *out = reinterpret_cast<uint32_t *>(desc) + (int64_t)f * cells;
    for (int c = threadIdx.x; c < cells; c += DESC_BLOCK) {
        const uint32_t v = img[c];
        if (parts == 1) out[c] = v;
        else if (v) atomicMax(out + c, v);
    }
}

// key [n][Nr], U [n][Nr * Ns], mask [n][2]; U and mask may be null (the descriptors alone)
__global__ __launch_bounds__(FIN_BLOCK) void place_finish_kernel(const float *__restrict__ desc, const PlaceParams o, float *__restrict__ key,
                                                                 double *__restrict__ U, uint64_t *__restrict__ mask)
{
    __shared__ float D[PLACE_MAX_RINGS * PLACE_MAX_SECTORS];
    const int nr = o.n_rings, ns = o.n_sectors, cells = nr * ns, t = threadIdx.x;
    const int64_t f = blockIdx.x;
    for (int c = t; c < cells; c += FIN_BLOCK) D[c] = desc[f * cells + c];
    __syncthreads();
    if (t < nr) key[f * nr + t] = place_ring_key(D + t * ns, ns);
    if (!U) return;
    bool full = false;
    if (t < ns) full = place_column(D, nr, ns, t, U + f * cells);
    const uint64_t m = __ballot(full ? 1 : 0);
    if ((t & 63) == 0) mask[2 * f + (t >> 6)] = m;
}

// pick [nq][K]: the frames of the K smallest (key distance, f) among the frames whose submap passes the gap clause, ascending; -1
// where there are fewer
__global__ __launch_bounds__(KEY_BLOCK) void place_key_kernel(int n, int nq, const float *__restrict__ key, const PlaceParams o,
                                                              int32_t *__restrict__ pick)
{
    __shared__ float d2s[KEY_BLOCK / 64][KEY_TILE];
    __shared__ PlaceKey top[KEY_BLOCK / 64][PLACE_MAX_K];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * (KEY_BLOCK / 64) + wv;
    if (q >= nq) return; // (the whole wavefront; the workgroup never synchronises, a lane reads back only what it wrote itself)
    const int j = (int)((int64_t)q * o.query_stride);
    const int nr = o.n_rings, K = o.n_key;
    const int64_t S = o.submap_size;
    const float *kq = key + (int64_t)j * nr;
    int kept = 0;                               // uniform
    PlaceKey worst; worst.d2 = INFINITY; worst.idx = INT32_MAX; // the K-th of the list once it is full (uniform)
    for (int t0 = 0; t0 < n; t0 += KEY_TILE) {
        const int t1 = t0 + KEY_TILE < n ? t0 + KEY_TILE : n;
        for (int f = t0 + lane; f < t1; f += 64) {
            const int64_t w = f / S;
            const int f0 = (int)(w * S), f1 = (int)(w * S + S < n ? w * S + S : n);
            d2s[wv][f - t0] = loop_gap_ok(j, f0, f1, o.min_gap) ? place_key_d2(kq, key + (int64_t)f * nr, nr) : INFINITY;
        }
        PlaceKey prev; prev.d2 = -1.0f; prev.idx = -1; // below every real pair
        for (int round = 0; round < K; ++round) {
            PlaceKey b; b.d2 = INFINITY; b.idx = INT32_MAX;
            for (int f = t0 + lane; f < t1; f += 64) {
                const float d2 = d2s[wv][f - t0];
                if (loop_less(prev.d2, prev.idx, d2, f) && loop_less(d2, f, b.d2, b.idx)) { b.d2 = d2; b.idx = f; }
            }
            b = wave_fold_to_lane63<MinPairStep<PlaceKey>>(b);
            prev.d2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b.d2), 63));
            prev.idx = __builtin_amdgcn_readlane(b.idx, 63);
            if (!(prev.d2 < INFINITY)) break;                                                    // the tile is exhausted
            if (kept == K && !loop_less(prev.d2, prev.idx, worst.d2, worst.idx)) break;          // nor does any later pick of it
            PlaceKey last = worst;
            if (lane == 0) {
                place_keep(top[wv], &kept, K, prev.d2, prev.idx);
                if (kept == K) last = top[wv][K - 1];
            }
            kept = __builtin_amdgcn_readfirstlane(kept);
            worst.d2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(last.d2)));
            worst.idx = __builtin_amdgcn_readfirstlane(last.idx);
        }
    }
    if (lane != 0) return;
    for (int a = 0; a < K; ++a) pick[(int64_t)q * K + a] = a < kept ? top[wv][a].idx : -1;
}

// dist, shift [nq][K] of the picks; grid nq * K, one wavefront each
__global__ __launch_bounds__(64) void place_shift_kernel(const int32_t *__restrict__ pick, const double *__restrict__ U,
                                                         const uint64_t *__restrict__ mask, const PlaceParams o, double *__restrict__ dist,
                                                         int32_t *__restrict__ shift)
{
    extern __shared__ double Us[]; // U_q, U_c
    const int lane = threadIdx.x, K = o.n_key, nr = o.n_rings, ns = o.n_sectors, cells = nr * ns;
    const int64_t e = blockIdx.x;
    const int f = pick[e];
    if (f < 0) {
        if (lane == 0) { dist[e] = 1.0; shift[e] = 0; }
        return;
    }
    const int64_t j = (e / K) * o.query_stride;
    for (int c = lane; c < cells; c += 64) {
        Us[c] = U[j * cells + c];
        Us[cells + c] = U[(int64_t)f * cells + c];
    }
    const uint64_t mq[2] = {mask[2 * j], mask[2 * j + 1]}, mc[2] = {mask[2 * (int64_t)f], mask[2 * (int64_t)f + 1]};
    __syncthreads();
    LoopBest b = loop_none();
    for (int s = lane; s < ns; s += 64) {
        const double d = place_dist_at(Us, Us + cells, mq, mc, nr, ns, s);
        if (loop_less(d, s, b.d2, b.idx)) { b.d2 = d; b.idx = s; }
    }
    b = wave_fold_to_lane63<MinPairStep<LoopBest>>(b);
    if (lane == 63) { dist[e] = b.d2; shift[e] = b.idx; }
}

// count [nq], stage [nq][max_per_frame]; one wavefront per query, lane = pick
__global__ __launch_bounds__(64) void place_select_kernel(const int32_t *__restrict__ pick, const double *__restrict__ dist,
                                                          const int32_t *__restrict__ shift, const PlaceParams o, int64_t *__restrict__ count,
                                                          lvba_place_candidate *__restrict__ stage)
{
    __shared__ int32_t f[PLACE_MAX_K];
    __shared__ double d[PLACE_MAX_K];
    __shared__ uint8_t eligible[PLACE_MAX_K], kept[PLACE_MAX_K];
    const int k = threadIdx.x, K = o.n_key, S = o.submap_size;
    const int64_t q = blockIdx.x;
    if (k < K) { f[k] = pick[q * K + k]; d[k] = dist[q * K + k]; }
    __syncthreads();
    if (k < K) eligible[k] = place_eligible(k, K, f, d, S, o.max_distance) ? 1 : 0;
    __syncthreads();
    if (k < K) kept[k] = place_kept(k, K, f, d, eligible, S, o.max_per_frame) ? 1 : 0;
    __syncthreads();
    const bool mine = k < K && kept[k];
    const uint64_t all = __ballot(mine ? 1 : 0);
    if (k == 0) count[q] = __popcll(all);
    if (!mine) return;
    lvba_place_candidate c;
    c.query = (int32_t)(q * o.query_stride); c.submap = f[k] / S; c.ref = f[k]; c.shift = shift[q * K + k];
    c.distance = d[k]; c.yaw = place_yaw(c.shift, o.n_sectors);
    stage[q * o.max_per_frame + place_slot(k, K, f, kept, S)] = c;
}

int32_t check_opts(const lvba_place_opts *opts, lvba_place_opts &o, PlaceParams &p)
{
    lvba_place_default_opts(&o);
    if (opts) o = *opts;
    const bool ok = o.n_rings >= 1 && o.n_rings <= PLACE_MAX_RINGS && o.n_sectors >= 1 && o.n_sectors <= PLACE_MAX_SECTORS &&
                    std::isfinite(o.min_range) && o.min_range >= 0.0 && std::isfinite(o.max_range) && o.max_range > o.min_range &&
                    std::isfinite(o.z_offset) && o.submap_size >= 1 && o.min_gap >= 0 && o.n_key_candidates >= 1 &&
                    o.n_key_candidates <= PLACE_MAX_K && o.max_per_frame >= 1 && o.max_per_frame <= LOOP_MAX_K && o.query_stride >= 1 &&
                    o.max_distance > 0.0 && o.max_distance <= 1.0;
    if (!ok)
        return lvba_fail(LVBA_ERR_ARG, "options: n_rings %d (1 .. %d), n_sectors %d (1 .. %d), min_range %g (>= 0), max_range %g (finite, > "
                         "min_range), z_offset %g (finite), submap_size %d (>= 1), min_gap %d (>= 0), n_key_candidates %d (1 .. %d), "
                         "max_per_frame %d (1 .. %d), query_stride %d (>= 1), max_distance %g (in (0, 1])", o.n_rings, PLACE_MAX_RINGS,
                         o.n_sectors, PLACE_MAX_SECTORS, o.min_range, o.max_range, o.z_offset, o.submap_size, o.min_gap, o.n_key_candidates,
                         PLACE_MAX_K, o.max_per_frame, LOOP_MAX_K, o.query_stride, o.max_distance);
    p.n_rings = o.n_rings; p.n_sectors = o.n_sectors; p.submap_size = o.submap_size; p.min_gap = o.min_gap; p.n_key = o.n_key_candidates;
    p.max_per_frame = o.max_per_frame; p.query_stride = o.query_stride;
    p.min_range = o.min_range; p.max_range = o.max_range; p.z_offset = o.z_offset; p.max_distance = o.max_distance;
    return LVBA_OK;
}

// the descriptors of frames [frame_begin, frame_begin + n) of `sc` into d_desc [n][Nr * Ns], on stream s (n > 0)
int32_t describe_dev(hipStream_t s, lvba_scans_s *sc, int frame_begin, int n, const PlaceParams &p, float *d_desc)
{
    int64_t most = 0;
    for (int f = 0; f < n; ++f) most = std::max(most, sc->frame_off[frame_begin + f + 1] - sc->frame_off[frame_begin + f]);
    const int parts = (int)std::min<int64_t>(DESC_MAX_PARTS, std::max<int64_t>(1, (most + DESC_PART_POINTS - 1) / DESC_PART_POINTS));
    const size_t cells = (size_t)p.n_rings * p.n_sectors;
    if (parts > 1) HIPCHK(hipMemsetAsync(d_desc, 0, 4 * cells * (size_t)n, s));
    place_describe_kernel<<<dim3(parts, n), DESC_BLOCK, 4 * cells, s>>>(sc->d_pts, sc->d_frame_off, frame_begin, p, d_desc);
    HIPCHK(hipGetLastError());
    return LVBA_OK;
}

// the search over descriptors d_desc [n][Nr * Ns] on the device, on stream s (n > 0)
int32_t search_dev(hipStream_t s, int n, const float *d_desc, const PlaceParams &p, int64_t capacity, lvba_place_candidate *out,
                   int64_t *count)
{
    const size_t cells = (size_t)p.n_rings * p.n_sectors, K = (size_t)p.n_key;
    const int nq = (int)(((int64_t)n + p.query_stride - 1) / p.query_stride);
    if ((int64_t)nq * p.n_key > INT32_MAX) return lvba_fail(LVBA_ERR_ARG, "%d queries x %d key candidates: more than 2^31 - 1 pairs", nq, p.n_key);
    DevArr<float> d_key(s); DevArr<double> d_U(s); DevArr<uint64_t> d_mask(s); DevArr<int32_t> d_pick(s); DevArr<double> d_dist(s);
    DevArr<int32_t> d_shift(s); DevArr<int64_t> d_count(s), d_first(s); DevArr<lvba_place_candidate> d_stage(s), d_out(s);
    HIPCHK(d_key.alloc((size_t)n * p.n_rings)); HIPCHK(d_U.alloc((size_t)n * cells)); HIPCHK(d_mask.alloc(2 * (size_t)n));
    HIPCHK(d_pick.alloc((size_t)nq * K)); HIPCHK(d_dist.alloc((size_t)nq * K)); HIPCHK(d_shift.alloc((size_t)nq * K));
    HIPCHK(d_count.alloc((size_t)nq + 1)); HIPCHK(d_first.alloc((size_t)nq + 1));
    HIPCHK(d_stage.alloc((size_t)nq * (size_t)p.max_per_frame));
    place_finish_kernel<<<n, FIN_BLOCK, 0, s>>>(d_desc, p, d_key, d_U, d_mask);
    HIPCHK(hipGetLastError());
    place_key_kernel<<<grid_for(nq, KEY_BLOCK / 64), KEY_BLOCK, 0, s>>>(n, nq, d_key, p, d_pick);
    HIPCHK(hipGetLastError());
    place_shift_kernel<<<(unsigned)((size_t)nq * K), 64, 16 * cells, s>>>(d_pick, d_U, d_mask, p,
                                                                        d_dist, d_shift);
    HIPCHK(hipGetLastError());
    HIPCHK(d_count.zero_async(1, nq));
    place_select_kernel<<<nq, 64, 0, s>>>(d_pick, d_dist, d_shift, p, d_count, d_stage);
    HIPCHK(hipGetLastError());
    TRY(scan_excl<int64_t>(s, d_count, d_first, (size_t)nq + 1));
    int64_t total = 0;
    HIPCHK(copy_d2h(&total, d_first + nq, d_first.bytes(1)));
    *count = total;
    const int64_t n_out = std::min(total, capacity);
    if (n_out == 0) return LVBA_OK;
    HIPCHK(d_out.alloc((size_t)n_out));
    loop_write_kernel<lvba_place_candidate><<<grid_for(nq, 256), 256, 0, s>>>(nq, p.max_per_frame, d_count, d_first,
                                                        d_stage, n_out, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(d_out.download(out, (size_t)n_out));
    return LVBA_OK;
}

} // namespace

extern "C" void lvba_place_default_opts(lvba_place_opts *o)
{
    if (!o) return;
    *o = lvba_place_opts{};
    o->n_rings = 20; o->n_sectors = 60;
    o->min_range = 0.5; o->max_range = 80.0; o->z_offset = 2.0;
    o->submap_size = 10; o->min_gap = 50; o->n_key_candidates = 10; o->max_per_frame = 2; o->query_stride = 1;
    o->max_distance = 0.4;
}

extern "C" int32_t lvba_place_descriptors(lvba_scans_t sc, int32_t frame_begin, int32_t n_frames, const lvba_place_opts *opts, float *desc,
                                          float *ring_key)
{
    if (!sc || n_frames < 0 || (n_frames > 0 && (!desc || !ring_key))) return lvba_fail(LVBA_ERR_ARG, "null argument or n_frames < 0");
    lvba_place_opts o;
    PlaceParams p;
    TRY(check_opts(opts, o, p));
    if (frame_begin < 0 || (int64_t)frame_begin + n_frames > sc->n_frames)
        return lvba_fail(LVBA_ERR_ARG, "frames [%d, %d + %d) of %d", frame_begin, frame_begin, n_frames, sc->n_frames);
    if (n_frames == 0) return LVBA_OK;
    const size_t cells = (size_t)p.n_rings * p.n_sectors, n = (size_t)n_frames;
    HIPCHK(hipSetDevice(sc->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<float> d_desc(sg.s), d_key(sg.s);
    HIPCHK(d_desc.alloc(n * cells)); HIPCHK(d_key.alloc(n * p.n_rings));
    TRY(describe_dev(sg.s, sc, frame_begin, n_frames, p, d_desc));
    place_finish_kernel<<<n_frames, FIN_BLOCK, 0, sg.s>>>(d_desc, p, d_key, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sg.s));
    HIPCHK(d_desc.download(desc, n * cells)); HIPCHK(d_key.download(ring_key, n * p.n_rings));
    return LVBA_OK;
}

extern "C" int32_t lvba_place_search(int32_t device, int32_t n_frames, const float *desc, const lvba_place_opts *opts, int64_t capacity,
                                     lvba_place_candidate *out, int64_t *count)
{
    if (!count || n_frames < 0 || capacity < 0 || (n_frames > 0 && !desc) || (capacity > 0 && !out))
        return lvba_fail(LVBA_ERR_ARG, "null argument, n_frames < 0 or capacity < 0");
    *count = 0;
    lvba_place_opts o;
    PlaceParams p;
    TRY(check_opts(opts, o, p));
    const size_t cells = (size_t)p.n_rings * p.n_sectors, n = (size_t)n_frames;
    for (size_t i = 0; i < n * cells; ++i)
        if (!(desc[i] >= 0.0f && desc[i] < INFINITY))
            return lvba_fail(LVBA_ERR_ARG, "frame %d: descriptor value %g (finite and >= 0)", (int)(i / cells), (double)desc[i]);
    if (n == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<float> d_desc(sg.s);
    HIPCHK(d_desc.alloc(n * cells)); HIPCHK(d_desc.upload(desc, n * cells));
    return search_dev(sg.s, n_frames, d_desc, p, capacity, out, count);
}

extern "C" int32_t lvba_place_candidates(lvba_scans_t sc, const lvba_place_opts *opts, int64_t capacity, lvba_place_candidate *out,
                                         int64_t *count)
{
    if (!sc || !count || capacity < 0 || (capacity > 0 && !out)) return lvba_fail(LVBA_ERR_ARG, "null argument or capacity < 0");
    *count = 0;
    lvba_place_opts o;
    PlaceParams p;
    TRY(check_opts(opts, o, p));
    const int n = sc->n_frames;
    if (n == 0) return LVBA_OK;
    HIPCHK(hipSetDevice(sc->device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<float> d_desc(sg.s);
    HIPCHK(d_desc.alloc((size_t)n * p.n_rings * p.n_sectors)); TRY(describe_dev(sg.s, sc, 0, n, p, d_desc));
    return search_dev(sg.s, n, d_desc, p, capacity, out, count);
}
