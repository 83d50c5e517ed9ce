// closures.hip -- pairwise consistency of loop closures: which closures agree with one another over the odometry between them, and
// a large set of mutually consistent ones (lvba_closure_consistency; the rule is in include/lvba_hip.h, its scalar arithmetic and
// bit-set steps in closure_device.h, also compiled for the host by the tests).
//
// Device design, six launches on one stream:
//   closure_prepare_kernel  a thread per closure: P_k = X_j Z_k^-1 X_i^-1 and t_i, component-major ([15][M]) so that the pair
//                           kernel's lanes read consecutive doubles.
//   closure_pair_kernel     one wavefront per (row a, word w), four to a workgroup; lane l is closure b = 64 w + l and evaluates the
//                           ordered pair (min, max) from the prepared form -- the side that is `a` is the same address in every lane
//                           (a broadcast), the other lane-consecutive.  The ballot of the decision is the adjacency word; lane 0
//                           stores it.  rot / trans are written when asked for.
//   closure_degree_kernel   one wavefront per row: popcounts over the words, an integer sum over the wavefront.
//   closure_seed_kernel     a thread per closure counts the closures that come before it in (degree descending, index ascending);
//                           that rank is its place among the seeds.  No reduction, no ties: the ranks are a permutation.
//   closure_set_kernel      one workgroup of sixteen wavefronts per seed; C and K in LDS.  Each round a wavefront takes the words
//                           of C it owns and, for every vertex v in them, counts |A[v] & C| (lanes over the words of the row, an
//                           integer sum over the wavefront); the wavefronts' best (count, v) go through LDS and every wavefront
//                           folds them to the round's pick (wave_fold_to_lane63 with MinPairStep on (-count, v)).  The owner of
//                           word v / 64 sets the bit of K, every thread updates its words of C.  When every vertex of C counted
//                           |C| the rest is a clique and is taken at once.
//   closure_select_kernel   one workgroup: the largest set, the first seed on a tie, into keep.
// No atomics anywhere, integer sums and lexicographic orders only: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "mempool.h"
#include "voxel_internal.h"
#include "closure_device.h"
#include "wave_ops.h"
#include "../../include/lvba_hip.h"

using namespace lvba;

namespace {

constexpr int PREP_BLOCK = 256;
constexpr int PAIR_BLOCK = 256;                 // four wavefronts, a word each
constexpr int DEG_BLOCK = 256;                  // four wavefronts, a row each
constexpr int SEED_BLOCK = 256;
constexpr int SET_BLOCK = 1024, SET_WAVES = SET_BLOCK / 64;
constexpr int SEL_BLOCK = 256;

struct ClosurePick { // (-count, v): the smallest pair is the largest count, the lowest v on a tie
    float d2;        // counts are <= 16384: exact
    int32_t idx;
};

__device__ __forceinline__ uint64_t readfirstlane_u64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// the integer sum of v over the wavefront, in every lane (all 64 lanes active)
__device__ __forceinline__ int wave_total(int v) { return __builtin_amdgcn_readlane(wave_fold_to_lane63<SumStepI32>(v), 63); }

// prep [CLOSURE_PREP][M]
__global__ __launch_bounds__(PREP_BLOCK) void closure_prepare_kernel(int M, const double *__restrict__ X, const int32_t *__restrict__ ref,
                                                                     const int32_t *__restrict__ query, const double *__restrict__ Z,
                                                                     double *__restrict__ prep)
{
    const int k = blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (k >= M) return;
    double Xi[12], Xj[12], Zk[12], out[CLOSURE_PREP];
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        Xi[c] = X[12 * (int64_t)ref[k] + c];
        Xj[c] = X[12 * (int64_t)query[k] + c];
        Zk[c] = Z[12 * (int64_t)k + c];
    }
    closure_prepare(Xi, Xj, Zk, out);
#pragma unroll
    for (int c = 0; c < CLOSURE_PREP; ++c) prep[(int64_t)c * M + k] = out[c];
}

// adj [M][W]; rot, trans [M][M] or null; grid (ceil(W / 4), M)
__global__ __launch_bounds__(PAIR_BLOCK) void closure_pair_kernel(int M, int W, const double *__restrict__ prep, const int32_t *__restrict__ ref,
                                                                  const int32_t *__restrict__ query, const ClosureParams o,
                                                                  uint64_t *__restrict__ adj, double *__restrict__ rot, double *__restrict__ trans)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * (PAIR_BLOCK / 64) + wv, a = blockIdx.y;
    if (w >= W) return; // (the whole wavefront; the workgroup never synchronises)
    const int b = 64 * w + lane;
    bool ok = false;
    if (b < M) {
        double r = 0.0, t = 0.0;
        if (a == b) {
            ok = true;
        } else {
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            double Pa[CLOSURE_PREP], Pb[12];
#pragma unroll
            for (int c = 0; c < CLOSURE_PREP; ++c) Pa[c] = prep[(int64_t)c * M + lo];
#pragma unroll
            for (int c = 0; c < 12; ++c) Pb[c] = prep[(int64_t)c * M + hi];
            closure_measures(Pa, Pb, &r, &t);
            ok = closure_consistent(r, t, closure_path(ref[lo], query[lo], ref[hi], query[hi]), o);
        }
        if (rot) rot[(int64_t)a * M + b] = r;
        if (trans) trans[(int64_t)a * M + b] = t;
    }
    const uint64_t word = __ballot(ok ? 1 : 0);
    if (lane == 0) adj[(int64_t)a * W + w] = word;
}

// deg [M] = popcount(A[v]) - 1
__global__ __launch_bounds__(DEG_BLOCK) void closure_degree_kernel(int M, int W, const uint64_t *__restrict__ adj, int32_t *__restrict__ deg)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int v = blockIdx.x * (DEG_BLOCK / 64) + wv;
    if (v >= M) return; // (the whole wavefront)
    const int c = wave_total(closure_row_bits(adj + (int64_t)v * W, lane, W, 64));
    if (lane == 0) deg[v] = c - 1;
}

// seeds [n_seeds]: the first n_seeds closures by (degree descending, index ascending)
__global__ __launch_bounds__(SEED_BLOCK) void closure_seed_kernel(int M, int n_seeds, const int32_t *__restrict__ deg, int32_t *__restrict__ seeds)
{
    const int v = blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (v >= M) return;
    const int32_t dv = deg[v];
    int rank = 0;
    for (int u = 0; u < M; ++u) rank += closure_before(deg[u], u, dv, v) ? 1 : 0; // deg[u]: the same address in every lane
    if (rank < n_seeds) seeds[rank] = v;
}

// sets [n_seeds][W], size [n_seeds]; one workgroup per seed
__global__ __launch_bounds__(SET_BLOCK) void closure_set_kernel(int M, int W, const uint64_t *__restrict__ adj, const int32_t *__restrict__ deg,
                                                                const int32_t *__restrict__ seeds, uint64_t *__restrict__ sets,
                                                                int32_t *__restrict__ size)
{
    __shared__ uint64_t Cs[CLOSURE_MAX_WORDS], Ks[CLOSURE_MAX_WORDS];
    __shared__ ClosurePick best[SET_WAVES];
    __shared__ int32_t full[SET_WAVES];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int32_t s = seeds[blockIdx.x];
    if (tid < W) { // W <= CLOSURE_MAX_WORDS < SET_BLOCK: thread w owns word w of C and K
        Cs[tid] = closure_take(adj[(int64_t)s * W + tid], ~(uint64_t)0, tid, s);
        Ks[tid] = closure_bit(tid, s);
    }
    int csize = deg[s], ksize = 1; // |C|, |K| (uniform)
    __syncthreads();
    while (csize > 0) {
        int32_t bc = -1, bv = INT32_MAX; // this wavefront's best (count, v) (uniform)
        bool all = true;                 // every vertex it saw counted |C|
        for (int w = wv; w < W; w += SET_WAVES) {
            uint64_t word = readfirstlane_u64(Cs[w]);
            while (word) {
                const int32_t v = 64 * w + __builtin_ctzll(word);
                word &= word - 1;
                const int32_t cnt = wave_total(closure_row_count(adj + (int64_t)v * W, Cs, lane, W, 64));
                if (closure_before(cnt, v, bc, bv)) { bc = cnt; bv = v; }
                all = all && cnt == csize;
            }
        }
        if (lane == 0) {
            best[wv].d2 = bc < 0 ? INFINITY : -(float)bc; best[wv].idx = bv;
            full[wv] = all ? 1 : 0;
        }
        __syncthreads();
        ClosurePick p;
        p.d2 = INFINITY; p.idx = INT32_MAX;
        if (lane < SET_WAVES) p = best[lane];
        const bool clique = __all(lane < SET_WAVES ? full[lane] : 1);
        if (clique) { // C is a clique: the rule would take all of it, one vertex a round
            if (tid < W) Ks[tid] |= Cs[tid];
            ksize += csize;
            break;
        }
        p = wave_fold_to_lane63<MinPairStep<ClosurePick>>(p);
        const int32_t v = __builtin_amdgcn_readlane(p.idx, 63);
        const int32_t cnt = -(int32_t)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.d2), 63));
        if (tid < W) {
            Cs[tid] = closure_take(Cs[tid], adj[(int64_t)v * W + tid], tid, v);
            Ks[tid] |= closure_bit(tid, v);
        }
        csize = cnt - 1; // v itself was counted
        ++ksize;
        __syncthreads();
    }
    if (tid < W) sets[(int64_t)blockIdx.x * W + tid] = Ks[tid]; // thread w wrote Ks[w] itself
    if (tid == 0) size[blockIdx.x] = ksize;
}

// keep [M], n_keep [1]: the largest set, the first seed on a tie; nothing when it has fewer than min_set members.  One workgroup.
__global__ __launch_bounds__(SEL_BLOCK) void closure_select_kernel(int M, int W, int n_seeds, int min_set, const uint64_t *__restrict__ sets,
                                                                   const int32_t *__restrict__ size, uint8_t *__restrict__ keep,
                                                                   int32_t *__restrict__ n_keep)
{
    const int lane = threadIdx.x & 63;
    int32_t bc = -1, bs = INT32_MAX; // every wavefront finds the same pair
    for (int s = lane; s < n_seeds; s += 64) {
        const int32_t c = size[s];
        if (closure_before(c, s, bc, bs)) { bc = c; bs = s; }
    }
    ClosurePick p;
    p.d2 = bc < 0 ? INFINITY : -(float)bc; p.idx = bs;
    p = wave_fold_to_lane63<MinPairStep<ClosurePick>>(p);
    const int32_t seed = __builtin_amdgcn_readlane(p.idx, 63);
    const int32_t cnt = -(int32_t)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.d2), 63));
    const bool any = cnt >= min_set;
    for (int v = threadIdx.x; v < M; v += SEL_BLOCK)
        keep[v] = any && ((sets[(int64_t)seed * W + (v >> 6)] >> (v & 63)) & 1) ? 1 : 0;
    if (threadIdx.x == 0) *n_keep = any ? cnt : 0;
}

bool rot_ok(const double *R) // the test of PriorTables (prior_tables.hip)
{
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - (a == b ? 1.0 : 0.0);
            if (!(fabs(d) <= 1e-6)) return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;
}

} // namespace

extern "C" void lvba_closure_default_opts(lvba_closure_opts *o)
{
    if (!o) return;
    *o = lvba_closure_opts{};
    o->rot_tol = 0.035; o->rot_rate = 0.001;
    o->trans_tol = 0.2; o->trans_rate = 0.01;
    o->n_seeds = 32; o->min_set = 2;
}

extern "C" int32_t lvba_closure_consistency(int32_t device, int32_t n_frames, const double *poses, int32_t n, const int32_t *ref,
                                            const int32_t *query, const double *meas, const lvba_closure_opts *opts, uint64_t *adjacency,
                                            double *rot, double *trans, uint8_t *keep, int32_t *n_keep)
{
    if (!n_keep || n < 0 || n > CLOSURE_MAX || (n > 0 && (!poses || !ref || !query || !meas || !keep)))
        return lvba_fail(LVBA_ERR_ARG, "null argument, or n %d outside 0 .. %d", n, CLOSURE_MAX);
    lvba_closure_opts o;
    lvba_closure_default_opts(&o);
    if (opts) o = *opts;
    const auto tol_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!tol_ok(o.rot_tol) || !tol_ok(o.rot_rate) || !tol_ok(o.trans_tol) || !tol_ok(o.trans_rate) || o.n_seeds < 1 || o.min_set < 1)
        return lvba_fail(LVBA_ERR_ARG, "options: rot_tol %g, rot_rate %g, trans_tol %g, trans_rate %g (finite and >= 0), n_seeds %d (>= 1), "
                         "min_set %d (>= 1)", o.rot_tol, o.rot_rate, o.trans_tol, o.trans_rate, o.n_seeds, o.min_set);
    if (n == 0) {
        *n_keep = 0;
        return LVBA_OK;
    }
    if (n_frames < 1) return lvba_fail(LVBA_ERR_ARG, "n_frames %d with %d closures", n_frames, n);
    for (int k = 0; k < n; ++k) {
        if (ref[k] < 0 || ref[k] >= n_frames || query[k] < 0 || query[k] >= n_frames)
            return lvba_fail(LVBA_ERR_ARG, "closure %d: frames (%d, %d) outside [0, %d)", k, ref[k], query[k], n_frames);
        if (ref[k] == query[k]) return lvba_fail(LVBA_ERR_ARG, "closure %d: a closure needs two different frames", k);
        for (int a = 0; a < 12; ++a)
            if (!std::isfinite(meas[12 * (size_t)k + a])) return lvba_fail(LVBA_ERR_ARG, "closure %d: non-finite measurement", k);
        if (!rot_ok(meas + 12 * (size_t)k)) return lvba_fail(LVBA_ERR_ARG, "closure %d: the measured rotation is not orthonormal", k);
    }
    for (size_t a = 0; a < 12 * (size_t)n_frames; ++a)
        if (!std::isfinite(poses[a])) return lvba_fail(LVBA_ERR_ARG, "frame %d: non-finite pose", (int)(a / 12));
    const int M = n, W = (M + 63) / 64, n_seeds = std::min(o.n_seeds, M);
    const size_t MM = (size_t)M * (size_t)M;
    ClosureParams par;
    par.rot_tol = o.rot_tol; par.rot_rate = o.rot_rate; par.trans_tol = o.trans_tol; par.trans_rate = o.trans_rate;
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    DevArr<double> d_X(s); DevArr<int32_t> d_ref(s), d_query(s); DevArr<double> d_Z(s), d_prep(s); DevArr<uint64_t> d_adj(s);
    DevArr<double> d_rot(s), d_trans(s); DevArr<int32_t> d_deg(s), d_seeds(s); DevArr<uint64_t> d_sets(s);
    DevArr<int32_t> d_size(s); DevArr<uint8_t> d_keep(s); DevArr<int32_t> d_nkeep(s);
    HIPCHK(d_X.alloc(12 * (size_t)n_frames)); HIPCHK(d_ref.alloc((size_t)M)); HIPCHK(d_query.alloc((size_t)M));
    HIPCHK(d_Z.alloc(12 * (size_t)M)); HIPCHK(d_prep.alloc((size_t)CLOSURE_PREP * M)); HIPCHK(d_adj.alloc((size_t)M * W));
    if (rot) HIPCHK(d_rot.alloc(MM));
    if (trans) HIPCHK(d_trans.alloc(MM));
    HIPCHK(d_deg.alloc((size_t)M)); HIPCHK(d_seeds.alloc((size_t)n_seeds)); HIPCHK(d_sets.alloc((size_t)n_seeds * W));
    HIPCHK(d_size.alloc((size_t)n_seeds)); HIPCHK(d_keep.alloc((size_t)M)); HIPCHK(d_nkeep.alloc(1));
    HIPCHK(d_X.upload(poses, 12 * (size_t)n_frames)); HIPCHK(d_ref.upload(ref, (size_t)M));
    HIPCHK(d_query.upload(query, (size_t)M)); HIPCHK(d_Z.upload(meas, 12 * (size_t)M));
    closure_prepare_kernel<<<grid_for(M, PREP_BLOCK), PREP_BLOCK, 0, s>>>(M, d_X, d_ref, d_query,
                                                                         d_Z, d_prep);
    HIPCHK(hipGetLastError());
    closure_pair_kernel<<<dim3(grid_for(W, PAIR_BLOCK / 64), M), PAIR_BLOCK, 0, s>>>(M, W, d_prep, d_ref,
                                                                                    d_query, par, d_adj,
                                                                                    rot ? d_rot : nullptr,
                                                                                    trans ? d_trans : nullptr);
    HIPCHK(hipGetLastError());
    closure_degree_kernel<<<grid_for(M, DEG_BLOCK / 64), DEG_BLOCK, 0, s>>>(M, W, d_adj, d_deg);
    HIPCHK(hipGetLastError());
    closure_seed_kernel<<<grid_for(M, SEED_BLOCK), SEED_BLOCK, 0, s>>>(M, n_seeds, d_deg, d_seeds);
    HIPCHK(hipGetLastError());
    closure_set_kernel<<<n_seeds, SET_BLOCK, 0, s>>>(M, W, d_adj, d_deg, d_seeds, d_sets, d_size);
    HIPCHK(hipGetLastError());
    closure_select_kernel<<<1, SEL_BLOCK, 0, s>>>(M, W, n_seeds, o.min_set, d_sets, d_size, d_keep, d_nkeep);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    // everything has run: only now is anything of the caller's written
    std::vector<uint8_t> h_keep((size_t)M);
    int32_t h_nkeep = 0;
    HIPCHK(d_keep.download(h_keep.data(), (size_t)M)); HIPCHK(d_nkeep.download(&h_nkeep, 1));
    if (adjacency) HIPCHK(d_adj.download(adjacency, (size_t)M * W));
    if (rot) HIPCHK(d_rot.download(rot, MM));
    if (trans) HIPCHK(d_trans.download(trans, MM));
    std::copy(h_keep.begin(), h_keep.end(), keep);
    *n_keep = h_nkeep;
    return LVBA_OK;
}
