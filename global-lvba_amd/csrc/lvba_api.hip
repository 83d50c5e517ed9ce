// lvba_api.hip -- BALM half of the C-ABI (include/lvba_hip.h): problem packing and the Nielsen-LM driver of
// BALM2::damping_iter (reference include/BALM/bavoxel.hpp:662-767; its damping rule is lm_rule.h).  Host logic only; all arithmetic on
// problem data runs in the kernels of balm_kernels.hip / ldlt.hip.  Shared machinery (ordering, assembly lists, solver,
// RCCL) lives in block_system.hip.  No CPU fallback.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "host_arena.h"
#include "block_system.h"
#include "host_tables.h"
#include "prior_tables.h"
#include "lm_rule.h"

using namespace lvba;

#define fail lvba_fail

// ------------------------------------------------------------------------------------------ handle
enum { EV_COST = 0, EV_EVAL, EV_SOLVE, EV_REDUCE, EV_COSTK, EV_EVALK, EV_N };

struct lvba_balm_s {
    BlockSys bs;
    int32_t N = 0;
    int64_t V = 0, F = 0, Q = 0, n_chunks = 0, Vglobal = 0;
    // host copies kept until finalize()
    lvba::hvec<int64_t> h_voff;
    lvba::hvec<int32_t> h_pidx;
    bool finalized = false;
    bool voxels_sorted = false; // the voxels were re-laid in the order of the first pose that sees them (balm_create_impl)
    int64_t *d_vox_order = nullptr; // then: voxel v of the handle's layout is voxel d_vox_order[v] of the caller's (lvba_balm_voxel_residuals)
    // robust loss on the voxel costs (lvba_balm_set_loss); TRIVIAL: none, the plain kernels run
    lvba_loss loss{LVBA_LOSS_TRIVIAL, 0, 0.0};
    bool loss_check = true;             // a sharded handle checks on its next collective call that every rank set the same loss
    // device data (voxel-major)
    int64_t *d_voff = nullptr, *d_chunk_v0 = nullptr;
    int32_t *d_pidx = nullptr;
    double *d_clu = nullptr, *d_chunk_cost = nullptr;
    // pose-major payload
    double *d_clu_csc = nullptr, *d_vrec = nullptr, *d_part = nullptr;
    double *d_pose_in = nullptr, *d_pose_cur = nullptr, *d_pose_trial = nullptr, *d_out = nullptr;
    double *d_scal2 = nullptr; // [0]=trial cost sum
    double *d_q1part = nullptr; // per-workgroup shares of the q1 numerator (retract_q1_kernel)
    double *h_pin = nullptr;   // pinned host staging, 16 doubles
    // grouped refinement (lvba_balm_set_groups): independent pose / voxel groups, one LM state each
    int32_t n_groups = 0;
    lvba::hvec<int32_t> g_pose_off;   // [n_groups + 1]
    lvba::hvec<int64_t> g_vox_off;    // [n_groups + 1]
    int32_t *d_grp_of_pose = nullptr, *d_gpo = nullptr, *d_gaccept = nullptr;
    int64_t *d_gco = nullptr;          // chunk range of every group
    double *d_gscal = nullptr;         // [3][n_groups]: cost at the current poses, cost at the trial poses, q1 numerator
    double *h_gpin = nullptr;          // pinned, [3][n_groups]
    int32_t *h_gacc = nullptr;         // pinned, [n_groups]
    // LM state (bavoxel.hpp:664-671): u, v, is_calc_hess, the iteration count and the stop flag are the rule's (lm_rule.h)
    bool lm_active = false;
    lvba_balm_opts lm_opts{};
    LmRule lm;
    double residual1 = 0.0;
    bool have_eval = false;
    // the voxel records (d_vrec) and chunk costs belong to the poses in d_pose_cur: the LM loop costs its trial point with the
    // voxel pass of the evaluation, and an accepted trial point is where the next evaluation happens
    bool lin_at_cur = false;
    // pose priors (lvba_balm_set_priors): as the caller gave them, and bound to the solver order (bind_priors)
    std::vector<lvba_prior> priors;
    bool prior_check = true;            // a sharded handle checks on its next collective call that every rank set the same priors
    PriorTables pt;                     // their records and scatter tables on the device (pt.dev.n == 0: none bound)
    lvba::hvec<int64_t> vox_slots;      // blocks the voxel evaluation writes (sorted; bind_priors)
    bool vox_slots_known = false, vox_all_add = false;
    lvba::hvec<int64_t> build_slots;    // blocks of relative priors bound when the store was laid out (sorted)
    // profiling
    bool prof_on = false;
    hipEvent_t ev[EV_N][2] = {};
    bool ev_used[EV_N] = {};
    lvba_prof_t prof{};

    hipStream_t stream() const { return bs.stream; }
    BalmDev dev() const
    {
        BalmDev d;
        d.n_poses = N; d.band_blocks = bs.Bb; d.V = V; d.F = F; d.n_chunks = n_chunks;
        d.voff = d_voff; d.pidx = d_pidx; d.clu = d_clu; d.chunk_v0 = d_chunk_v0;
        d.S = bs.S; d.csc_off = bs.d_csc_off; d.clu_csc = d_clu_csc; d.vox_of_pos = bs.d_group_of_pos; d.vrec = d_vrec;
        d.Y = bs.d_Y; d.part = d_part;
        d.loss_kind = loss.kind; d.loss_scale = loss.scale;
        return d;
    }
};

// ------------------------------------------------------------------------------------------ misc API
extern "C" int32_t lvba_version(void) { return 112; }
extern "C" int32_t lvba_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" void lvba_balm_default_opts(lvba_balm_opts *o)
{
    if (!o) return;
    o->max_iter = 10; o->reserved = 0; o->u0 = 0.01; o->v0 = 2.0; o->rel_tol = 1e-6;
}
extern "C" void lvba_shard_range(int64_t V, int32_t rank, int32_t G, int64_t *head, int64_t *end)
{
    if (G < 1) G = 1;
    // exact integer floor(V*r/G); the reference's double arithmetic agrees for V < 2^53/G
    if (head) *head = (int64_t)(((__int128)V * rank) / G);
    if (end) *end = (int64_t)(((__int128)V * (rank + 1)) / G);
}

// ------------------------------------------------------------------------------------------ create
static int32_t balm_create_impl(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off, const int32_t *pose_idx,
                                const double *clusters, const double *d_clusters, int32_t device, lvba_balm_t *out, bool trusted = false);

extern "C" int32_t lvba_balm_create(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off,
                                    const int32_t *pose_idx, const double *clusters, int32_t device,
                                    lvba_balm_t *out)
{
    return balm_create_impl(n_poses, n_voxels, voxel_off, pose_idx, clusters, nullptr, device, out);
}

// (internal, window_ba.hip) the caller vouches for its arrays -- they come out of this library's own voxel maps: no range checks,
// no voxel re-layout pass (1.1 of the 7.3 ms the joint LM of bench.py's window leg took)
namespace lvba {
int32_t balm_create_dev_trusted(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off, const int32_t *pose_idx,
                                const double *d_clusters, int32_t device, lvba_balm_t *out)
{
    if (!d_clusters) return fail(LVBA_ERR_ARG, "d_clusters is NULL");
    return balm_create_impl(n_poses, n_voxels, voxel_off, pose_idx, nullptr, d_clusters, device, out, true);
}
} // namespace lvba

extern "C" int32_t lvba_balm_create_dev(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off, const int32_t *pose_idx,
                                        const double *d_clusters, int32_t device, lvba_balm_t *out)
{
    return balm_create_impl(n_poses, n_voxels, voxel_off, pose_idx, nullptr, d_clusters, device, out);
}

static int32_t balm_create_impl(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off, const int32_t *pose_idx,
                                const double *clusters, const double *d_clusters, int32_t device, lvba_balm_t *out, bool trusted)
{
    if (!out) return fail(LVBA_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n_poses < 1 || n_voxels < 1 || !voxel_off || !pose_idx || (!clusters && !d_clusters))
        return fail(LVBA_ERR_ARG, "n_poses/n_voxels must be >= 1 and arrays non-NULL");
    const int64_t base = voxel_off[0];
    const int64_t F = voxel_off[n_voxels] - base;
    if (F < 2 * n_voxels) return fail(LVBA_ERR_ARG, "every voxel needs >= 2 factors (push_voxel, bavoxel.hpp:52)");
    if (F >= (int64_t)1 << 31) return fail(LVBA_ERR_UNSUPPORTED, "more than 2^31 factors per shard");
    TRY(lvba::check_device(device));

    const bool timing = timing_on("build");
    auto nowc = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tmark = nowc();
    auto mark = [&](const char *what) {
        if (!timing) return;
        const double t = nowc();
        fprintf(stderr, "[balm_create] %-14s %.3f ms\n", what, t - tmark);
        tmark = t;
    };
    // one pass over the voxels: >= 2 factors each, pose indices in range, and the first pose that sees each voxel (for the
    // re-layout decision below; only needed from the size on from which the pair lists are windowed)
    const bool want_key = !trusted && 18 * 8 * F > ((int64_t)24 << 20) && n_voxels > 1;
    lvba::hvec<int32_t> key;
    if (want_key) key.resize((size_t)n_voxels);
    double jump = 0.0;
    for (int64_t a = 0; a < (trusted ? 0 : n_voxels); ++a) { // (trusted: the window driver's own voxel maps, window_ba.hip)
        const int64_t f0 = voxel_off[a] - base, f1 = voxel_off[a + 1] - base;
        if (f1 - f0 < 2) return fail(LVBA_ERR_ARG, "voxel %lld has %lld factors (< 2)", (long long)a, (long long)(f1 - f0));
        int32_t lo = 0x7fffffff, hi = -1;
        for (int64_t f = f0; f < f1; ++f) { lo = std::min(lo, pose_idx[f]); hi = std::max(hi, pose_idx[f]); }
        if (lo < 0 || hi >= n_poses) {
            for (int64_t f = f0; f < f1; ++f)
                if (pose_idx[f] < 0 || pose_idx[f] >= n_poses) return fail(LVBA_ERR_ARG, "pose_idx[%lld] = %d out of range", (long long)f, pose_idx[f]);
        }
        if (want_key) {
            key[(size_t)a] = lo;
            if (a > 0) jump += std::abs((double)lo - (double)key[(size_t)a - 1]);
        }
    }

    // Voxel order.  Every pass over the voxels is laid out for voxels that come roughly in the order of the poses that see
    // them (a voxel map built along a trajectory does; the synthetic problems do): the pose gather of the voxel pass, the
    // voxel records the factor pass gathers and above all the windows of the pair lists draw on a compact slice of memory then.
    // The reference hands its voxels over in the iteration order of an unordered_map (src/lvba_system.cpp:254-262 -> tras_opt),
    // i.e. in no order at all: at C3 that costs 17 % of the evaluation (2.71 vs 2.32 ms, tools/gpu_shuffled.sh).  So a large
    // problem whose voxels jump about is re-laid internally, voxels sorted (stably) by the first pose that sees them.  The
    // one output indexed by voxel, lvba_balm_voxel_residuals, goes back through the permutation kept for it (d_vox_order); sums
    // over voxels change in the last bits only.
    lvba::hvec<int64_t> voff_s;
    lvba::hvec<int32_t> pidx_s, fmap;
    lvba::hvec<int64_t> vox_order; // [new] = old, kept for the per-voxel outputs (lvba_balm_voxel_residuals)
    {
        const bool sort_voxels = want_key && jump / (double)(n_voxels - 1) > std::max(64.0, 0.125 * n_poses);
        if (sort_voxels) { // stable counting sort by the first pose
            lvba::hvec<int64_t> start((size_t)n_poses + 1, 0);
            for (int64_t a = 0; a < n_voxels; ++a) ++start[(size_t)key[(size_t)a] + 1];
            for (int32_t i = 0; i < n_poses; ++i) start[(size_t)i + 1] += start[(size_t)i];
            lvba::hvec<int64_t> order((size_t)n_voxels); // order[new] = old
            for (int64_t a = 0; a < n_voxels; ++a) order[(size_t)start[(size_t)key[(size_t)a]]++] = a;
            voff_s.resize((size_t)n_voxels + 1);
            pidx_s.resize((size_t)F);
            fmap.resize((size_t)F);
            voff_s[0] = 0;
            int64_t w = 0;
            for (int64_t a = 0; a < n_voxels; ++a) {
                const int64_t o = order[(size_t)a];
                for (int64_t f = voxel_off[o] - base; f < voxel_off[o + 1] - base; ++f, ++w) {
                    pidx_s[(size_t)w] = pose_idx[f];
                    fmap[(size_t)w] = (int32_t)f;
                }
                voff_s[(size_t)a + 1] = w;
            }
            voxel_off = voff_s.data();
            pose_idx = pidx_s.data();
            vox_order.swap(order);
        }
    }
    const int64_t base2 = voxel_off[0]; // 0 after a re-layout
    mark("checks + order");

    lvba_balm_s *h = new (std::nothrow) lvba_balm_s();
    if (!h) return fail(LVBA_ERR_NOMEM, "host allocation failed");
    h->N = n_poses; h->V = n_voxels; h->F = F; h->Vglobal = n_voxels;
    h->voxels_sorted = !fmap.empty();
    // validate + chunk
    h->h_voff.resize(n_voxels + 1);
    lvba::hvec<int64_t> chunk_v0;
    int64_t Q = 0;
    for (int64_t a = 0; a <= n_voxels; ++a) h->h_voff[a] = voxel_off[a] - base2;
    {
        const int64_t bad = lvba::chunk_voxels(n_voxels, voxel_off, LVBA_CF, LVBA_CV, chunk_v0, Q); // host_tables.h
        if (bad >= 0) {
            const long long k = (long long)(voxel_off[bad + 1] - voxel_off[bad]);
            delete h;
            return fail(LVBA_ERR_ARG, "voxel %lld has %lld factors (< 2)", (long long)bad, k);
        }
    }
    h->n_chunks = (int64_t)chunk_v0.size() - 1;
    h->Q = Q;
    h->h_pidx.assign(pose_idx, pose_idx + F);
    mark("chunks + copies");

    auto bail = [&](int32_t rc) { lvba_balm_destroy(h); return rc; };
#define CTRY(expr) do { int32_t rc_ = (expr); if (rc_ != LVBA_OK) return bail(rc_); } while (0)
#define CHIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(e_ == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    CTRY(bs_init(h->bs, device));
    BlockSys &bs = h->bs;
    CTRY(bs_dmalloc(bs, &h->d_voff, n_voxels + 1));
    CTRY(bs_dmalloc(bs, &h->d_chunk_v0, h->n_chunks + 1));
    CTRY(bs_dmalloc(bs, &h->d_pidx, F));
    CTRY(bs_dmalloc(bs, &h->d_clu, 10 * F));
    CTRY(bs_dmalloc(bs, &h->d_chunk_cost, h->n_chunks));
    CHIP(lvba::copy_h2d(h->d_voff, h->h_voff.data(), (size_t)(n_voxels + 1) * sizeof(int64_t)));
    CHIP(lvba::copy_h2d(h->d_chunk_v0, chunk_v0.data(), (size_t)(h->n_chunks + 1) * sizeof(int64_t)));
    if (!vox_order.empty()) {
        CTRY(bs_dmalloc(bs, &h->d_vox_order, n_voxels));
        CHIP(lvba::copy_h2d(h->d_vox_order, vox_order.data(), (size_t)n_voxels * sizeof(int64_t)));
    }
    { // AoS [F][10] -> SoA [10][F] on the device (a host array is staged in a temporary device buffer), through the factor map of
      // a re-layout
        const double *src = d_clusters; // like the host array: indexed relative to voxel_off[0]
        double *d_stage = nullptr;
        int32_t *d_fmap = nullptr;
        if (!d_clusters) {
            CTRY(bs_dmalloc(bs, &d_stage, 10 * F));
            CHIP(lvba::copy_h2d(d_stage, clusters, (size_t)(10 * F) * sizeof(double)));
            src = d_stage;
        }
        if (!fmap.empty()) {
            CTRY(bs_dmalloc(bs, &d_fmap, F));
            CHIP(lvba::copy_h2d(d_fmap, fmap.data(), (size_t)F * sizeof(int32_t)));
        }
        launch_aos_to_soa(src, d_fmap, F, h->d_clu, bs.stream);
        CHIP(hipGetLastError());
        CHIP(hipStreamSynchronize(bs.stream));
        if (d_stage) { lvba::DevicePool::get().free(d_stage); bs.device_bytes -= (int64_t)(10 * F) * (int64_t)sizeof(double); }
        if (d_fmap) { lvba::DevicePool::get().free(d_fmap); bs.device_bytes -= (int64_t)F * (int64_t)sizeof(int32_t); }
    }
    mark("device arrays");
    CHIP(lvba::PinnedCache::get().acquire((void **)&h->h_pin, 4096)); // (16 doubles; one size for the cache's sake)
    for (int e = 0; e < EV_N; ++e)
        for (int s = 0; s < 2; ++s) CHIP(hipEventCreate(&h->ev[e][s]));
    mark("pinned + events");
#undef CTRY
#undef CHIP
    *out = h;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_destroy(lvba_balm_t h)
{
    if (!h) return LVBA_OK;
    hipSetDevice(h->bs.device);
    if (h->bs.stream) hipStreamSynchronize(h->bs.stream);
    void *ptrs[] = {h->d_voff, h->d_chunk_v0, h->d_pidx, h->d_clu, h->d_chunk_cost, h->d_clu_csc, h->d_vrec, h->d_part,
                    h->d_pose_in, h->d_pose_cur, h->d_pose_trial, h->d_out, h->d_scal2, h->d_q1part, h->d_grp_of_pose, h->d_gpo, h->d_gaccept, h->d_gco,
                    h->d_gscal, h->d_vox_order};
    for (void *p : ptrs)
        if (p) lvba::DevicePool::get().free(p);
    h->pt.free_mem();
    lvba::PinnedCache::get().release(h->h_pin);
    lvba::PinnedCache::get().release(h->h_gpin);
    lvba::PinnedCache::get().release(h->h_gacc);
    for (int e = 0; e < EV_N; ++e)
        for (int s = 0; s < 2; ++s)
            if (h->ev[e][s]) hipEventDestroy(h->ev[e][s]);
    bs_destroy(h->bs);
    delete h;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_configure(lvba_balm_t h, int32_t ordering, double band_frac)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    if (h->finalized) return fail(LVBA_ERR_STATE, "configure must precede the first cost/eval/refine call");
    if (ordering != 0 && ordering != 1) return fail(LVBA_ERR_ARG, "ordering must be 0 or 1");
    if (!(band_frac >= 0.0)) return fail(LVBA_ERR_ARG, "band_frac must be >= 0");
    // a grouped problem keeps the caller's pose order: the per-group tables (damping, q1, accept / select) are indexed by it
    if (h->n_groups > 0 && ordering != 0) return fail(LVBA_ERR_STATE, "a grouped problem (lvba_balm_set_groups) keeps ordering 0");
    h->bs.ordering = ordering;
    h->bs.band_frac = band_frac;
    return LVBA_OK;
}

static int32_t prior_sync(lvba_balm_s *h);
static int32_t loss_sync(lvba_balm_s *h);
static int32_t bind_priors(lvba_balm_s *h);

static int32_t finalize(lvba_balm_s *h)
{
    // priors whose binding failed (out of memory) are bound again on the next call, never silently left out
    if (h->finalized) return h->pt.dev.n == (int32_t)h->priors.size() ? LVBA_OK : bind_priors(h);
    TRY(prior_sync(h)); // (before bs_build: the relative priors shape the store on every rank)
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    const int N = h->N;
    if (h->n_groups > 0) bs.ordering = 0; // (lvba_balm_configure / dist_init refuse to undo it; kept here as the single point of truth)
    const bool timing = timing_on("build");
    auto nowc = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tmark = nowc();
    auto mark = [&](const char *what) {
        if (!timing) return;
        const double t = nowc();
        fprintf(stderr, "[finalize] %-14s %.3f ms\n", what, t - tmark);
        tmark = t;
    };
    TRY(bs_build(bs, N, h->V, h->h_voff.data(), h->h_pidx.data()));
    { // experiment (round 4): fp32 Y records between the factor and the pair pass -- the column kernel's lists only
        const char *e = getenv("LVBA_Y32");
        bs.y32 = bs.pair_col && e && !strcmp(e, "1");
    }
    mark("bs_build");
    lvba::hvec<int32_t> p((size_t)h->F); // pose indices of the factors in solver order
    for (int64_t f = 0; f < h->F; ++f) p[f] = bs.iperm[h->h_pidx[f]];
    HIPCHK(lvba::copy_h2d(h->d_pidx, p.data(), (size_t)h->F * sizeof(int32_t)));
    mark("pose indices");
    TRY(bs_dmalloc(bs, &h->d_clu_csc, 10 * h->F));
    TRY(bs_dmalloc(bs, &h->d_vrec, 16 * h->V));
    TRY(bs_dmalloc(bs, &h->d_part, (int64_t)N * bs.S * 32));
    launch_gather_csc(h->d_clu, bs.d_csc_f, h->F, h->d_clu_csc, bs.stream);
    TRY(bs_dmalloc(bs, &h->d_pose_in, 12 * (int64_t)N));
    TRY(bs_dmalloc(bs, &h->d_pose_cur, 12 * (int64_t)N));
    TRY(bs_dmalloc(bs, &h->d_pose_trial, 12 * (int64_t)N));
    TRY(bs_dmalloc(bs, &h->d_out, 12 * (int64_t)N));
    TRY(bs_dmalloc(bs, &h->d_scal2, 8));
    TRY(bs_dmalloc(bs, &h->d_q1part, (N + 127) / 128 + 8));
    HIPCHK(hipStreamSynchronize(bs.stream));
    mark("pose-major copy");
    lvba::hvec<int64_t>().swap(h->h_voff);
    lvba::hvec<int32_t>().swap(h->h_pidx);
    h->finalized = true;
    if (!h->priors.empty()) {
        TRY(bind_priors(h));
        for (const int64_t q : h->bs.extra_slots) h->build_slots.push_back(q);
        std::sort(h->build_slots.begin(), h->build_slots.end());
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_info(lvba_balm_t h, lvba_balm_info_t *info)
{
    if (!h || !info) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    info->n_poses = h->N; info->n_ranks = h->bs.n_ranks; info->n_voxels = h->V; info->n_voxels_global = h->Vglobal;
    info->n_factors = h->F; info->n_pairs = h->Q; info->n_chunks = h->n_chunks; info->n_blocks = h->bs.nnzb;
    info->band_blocks = h->bs.Bb; info->use_band = h->bs.use_band ? 1 : 0; info->hess_bytes = h->bs.hblk_doubles * 8;
    info->device_bytes = h->bs.device_bytes;
    info->twist_panels = (h->bs.d_bcr || h->bs.nd.active) ? 0 : (int32_t)ldlt_twist_panels(h->bs.A.n, h->bs.A.ld, h->bs.A.bw);
    info->nd_kind = !h->bs.nd.active ? 0 : !strcmp(h->bs.nd.kind, "hubs") ? 1 : 2;
    info->nd_arcs = (int32_t)h->bs.nd.arcs.size(); info->nd_sep_poses = h->bs.nd.Ns; info->nd_sep_band_blocks = h->bs.nd.BbS;
    info->nd_model_band_ms = 1e3 * h->bs.nd.t_band; info->nd_model_nd_ms = 1e3 * h->bs.nd.t_nd;
    info->solve_ranks = !(h->bs.distributed() && h->bs.n_ranks >= 2) ? 1 : h->bs.nd.active ? h->bs.n_ranks : info->twist_panels > 0 ? 2 : 1;
    info->trial_linearised = 1;
    info->y_fp32 = h->bs.y32 ? 1 : 0;
    info->allreduce_bytes = !h->bs.distributed() ? 0 : 8 * ((h->bs.d_ar_slot ? 36 * h->bs.n_ar : h->bs.hblk_doubles) + 6 * (int64_t)h->N + 1);
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_pair_layout(lvba_balm_t h, lvba_pair_layout_t *out, int64_t *item_len, int64_t *item_slot, int64_t cap)
{
    if (!h || !out) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    return bs_pair_layout(h->bs, out, item_len, item_slot, cap);
}

extern "C" int32_t lvba_balm_eval_layout(lvba_balm_t h, lvba_eval_layout_t *out)
{
    if (!h || !out) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    const BalmDev d = h->dev();
    memset(out, 0, sizeof *out);
    out->slices = d.S; out->unit_form = 0; out->units = (int64_t)d.n_poses * d.S; out->unit_grid = balm_factor_grid(d);
    out->n_groups = d.V; out->n_factors = d.F; out->n_chunks = d.n_chunks;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_get_ordering(lvba_balm_t h, int32_t *perm)
{
    if (!h || !perm) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    memcpy(perm, h->bs.perm.data(), (size_t)h->N * sizeof(int32_t));
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_nd_model(lvba_balm_t h, int32_t n_ranks, lvba_nd_model_t *out)
{
    if (!h || !out || n_ranks < 1) return fail(LVBA_ERR_ARG, "bad argument");
    TRY(finalize(h));
    memset(out, 0, sizeof *out);
    out->n_ranks = n_ranks;
    double tb = 0.0, tn = 0.0;
    const int32_t rc = bs_nd_model(h->bs, n_ranks, &tb, &tn, &out->arcs, &out->sep_poses, &out->sep_band_blocks, &out->max_arc_poses,
                                   &out->max_arc_band_blocks);
    if (rc != LVBA_OK) return fail(rc, "no co-visibility graph was kept for this problem (fewer than 256 poses, grouped, or solved dense without an ordering)");
    out->band_ms = 1e3 * tb; out->nd_ms = 1e3 * tn;
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ profiling
static void ev_begin(lvba_balm_s *h, int which)
{
    if (h->prof_on) hipEventRecord(h->ev[which][0], h->stream());
}
static void ev_end(lvba_balm_s *h, int which)
{
    if (h->prof_on) { hipEventRecord(h->ev[which][1], h->stream()); h->ev_used[which] = true; }
}
static void ev_collect(lvba_balm_s *h) // call after a stream synchronize
{
    if (!h->prof_on) return;
    double *acc[EV_N] = {&h->prof.cost_ms, &h->prof.eval_ms, &h->prof.solve_ms, &h->prof.reduce_ms,
                         &h->prof.cost_kernel_ms, &h->prof.eval_kernel_ms};
    int64_t *cnt[EV_N] = {&h->prof.cost_calls, &h->prof.eval_calls, &h->prof.solve_calls, &h->prof.reduce_calls, nullptr, nullptr};
    for (int e = 0; e < EV_N; ++e)
        if (h->ev_used[e]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->ev[e][0], h->ev[e][1]) == hipSuccess) {
                *acc[e] += ms;
                if (cnt[e]) *cnt[e] += 1;
            }
            h->ev_used[e] = false;
        }
}
extern "C" int32_t lvba_balm_set_profiling(lvba_balm_t h, int32_t enable)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    h->prof_on = enable != 0;
    return LVBA_OK;
}
extern "C" int32_t lvba_balm_get_profile(lvba_balm_t h, lvba_prof_t *out, int32_t reset)
{
    if (!h || !out) return fail(LVBA_ERR_ARG, "NULL argument");
    *out = h->prof;
    if (reset) memset(&h->prof, 0, sizeof h->prof);
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ stages
// enqueue: cost at device poses (solver order) -> dst[0] = (global) sum of lambda_min
// with_lin: by the voxel pass of the evaluation instead of the cost-only kernel -- the same chunk costs, plus the voxel records
// at `poses`, which enqueue_eval can start from
static int32_t enqueue_cost(lvba_balm_s *h, const double *d_poses, double *dst, bool with_lin = false)
{
    ev_begin(h, EV_COST);
    launch_cost(h->dev(), d_poses, h->d_chunk_cost, dst, h->stream(), h->prof_on ? h->ev[EV_COSTK][0] : nullptr,
                h->prof_on ? h->ev[EV_COSTK][1] : nullptr, with_lin);
    if (h->prof_on) h->ev_used[EV_COSTK] = true;
    ev_end(h, EV_COST);
    if (h->bs.distributed()) {
        ev_begin(h, EV_REDUCE);
        TRY(bs_allreduce(h->bs, dst, 1));
        ev_end(h, EV_REDUCE);
    }
    launch_prior_cost(h->pt.dev, d_poses, dst, nullptr, h->stream()); // after the all-reduce: every rank adds them once
    HIPCHK(hipGetLastError());
    return LVBA_OK;
}

// enqueue: H, g, cost at device poses -> bs.d_hg (all-reduced over ranks)
// lin_in_place: the voxel records and chunk costs at d_poses are already there (enqueue_cost with_lin at the same poses)
static int32_t enqueue_eval(lvba_balm_s *h, const double *d_poses, bool lin_in_place = false)
{
    BlockSys &bs = h->bs;
    ev_begin(h, EV_EVAL);
    TRY(bs_clear_reduced(bs));
    launch_eval(h->dev(), bs.pair_dev(), d_poses, bs.Hblk(), bs.hblk_doubles, bs.g(), h->d_chunk_cost, bs.scal(),
                false, bs.stream, h->prof_on ? h->ev[EV_EVALK][0] : nullptr,
                h->prof_on ? h->ev[EV_EVALK][1] : nullptr, lin_in_place);
    if (h->prof_on) h->ev_used[EV_EVALK] = true;
    ev_end(h, EV_EVAL);
    if (bs.distributed()) {
        ev_begin(h, EV_REDUCE);
        TRY(bs_allreduce_hg(bs));
        ev_end(h, EV_REDUCE);
    }
    launch_prior_eval(h->pt.dev, d_poses, bs.Hblk(), bs.g(), bs.scal(), bs.stream); // after the all-reduce: every rank adds them once
    HIPCHK(hipGetLastError());
    h->have_eval = true;
    return LVBA_OK;
}

static int32_t enqueue_solve(lvba_balm_s *h, double u)
{
    ev_begin(h, EV_SOLVE);
    TRY(bs_enqueue_solve(h->bs, u));
    ev_end(h, EV_SOLVE);
    return LVBA_OK;
}

// poses of the solver's order on the device -> caller's order on the host
static int32_t download_poses(lvba_balm_s *h, const double *d_src, double *poses_out)
{
    const size_t bytes = (size_t)12 * h->N * sizeof(double);
    if (bytes <= lvba::HostStage::kBytes) { // zero-copy, like upload_poses
        if (void *st = lvba::HostStage::get().lock(bytes)) {
            launch_export_poses(d_src, h->bs.d_perm, h->N, static_cast<double *>(st), h->stream());
            const hipError_t e = hipStreamSynchronize(h->stream());
            if (e == hipSuccess) memcpy(poses_out, st, bytes);
            lvba::HostStage::get().unlock(st);
            HIPCHK(e);
            return LVBA_OK;
        }
    }
    launch_export_poses(d_src, h->bs.d_perm, h->N, h->d_out, h->stream());
    HIPCHK(hipStreamSynchronize(h->stream()));
    HIPCHK(lvba::copy_d2h(poses_out, h->d_out, bytes));
    return LVBA_OK;
}

static int32_t upload_poses(lvba_balm_s *h, const double *poses, double *d_dst)
{
    const size_t bytes = (size_t)12 * h->N * sizeof(double);
    if (bytes <= lvba::HostStage::kBytes) { // zero-copy through the process-wide pinned stage (mempool.h)
        if (void *st = lvba::HostStage::get().lock(bytes)) {
            memcpy(st, poses, bytes);
            launch_import_poses(static_cast<const double *>(st), h->bs.d_perm, h->N, d_dst, h->stream());
            const hipError_t e = hipStreamSynchronize(h->stream()); // the kernel has read the stage
            lvba::HostStage::get().unlock(st);
            HIPCHK(e);
            return LVBA_OK;
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream())); // d_pose_in may still be read by an earlier import
    HIPCHK(lvba::copy_h2d(h->d_pose_in, poses, bytes));
    launch_import_poses(h->d_pose_in, h->bs.d_perm, h->N, d_dst, h->stream());
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ a7 / a6
extern "C" int32_t lvba_balm_cost(lvba_balm_t h, const double *poses, int32_t is_avg, double *cost)
{
    if (!h || !poses || !cost) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    TRY(prior_sync(h));
    TRY(loss_sync(h));
    HIPCHK(hipSetDevice(h->bs.device));
    TRY(upload_poses(h, poses, h->d_pose_trial));
    h->lin_at_cur = false; // the chunk costs are overwritten
    TRY(enqueue_cost(h, h->d_pose_trial, h->d_scal2));
    HIPCHK(hipMemcpyAsync(h->h_pin, h->d_scal2, sizeof(double), hipMemcpyDeviceToHost, h->stream()));
    HIPCHK(hipStreamSynchronize(h->stream()));
    ev_collect(h);
    *cost = is_avg ? h->h_pin[0] / (double)h->Vglobal : h->h_pin[0];
    if (!isfinite(*cost)) return fail(LVBA_NUM_NONFINITE, "non-finite cost");
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_eval(lvba_balm_t h, const double *poses, double *H, double *g, double *cost_avg)
{
    if (!h || !poses) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    TRY(prior_sync(h));
    TRY(loss_sync(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(upload_poses(h, poses, h->d_pose_cur));
    h->lin_at_cur = false; // (a full evaluation; an LM loop in progress starts its next evaluation from scratch too)
    TRY(enqueue_eval(h, h->d_pose_cur));
    HIPCHK(hipMemcpyAsync(h->h_pin, bs.scal(), sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    const int64_t n = 6 * (int64_t)h->N;
    if (g) {
        launch_export_vec(bs.g(), bs.d_perm, h->N, h->d_out, bs.stream);
        HIPCHK(hipMemcpyAsync(g, h->d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    }
    DevArr<double> dH(bs.stream); // freed on every path, error returns included
    if (H) {
        HIPCHK(dH.alloc((size_t)(n * n)));
        launch_export_dense(bs.Hblk(), bs.Bb, h->N, bs.d_perm, dH, bs.stream);
        HIPCHK(hipMemcpyAsync(H, dH, dH.bytes((size_t)(n * n)), hipMemcpyDeviceToHost, bs.stream));
    }
    HIPCHK(hipStreamSynchronize(bs.stream));
    ev_collect(h);
    if (cost_avg) *cost_avg = h->h_pin[0] / (double)h->Vglobal;
    return LVBA_OK;
}

// H of an evaluation in sparse form (the dense matrix of lvba_balm_eval is 28.8 GB at 10 000 poses): see include/lvba_hip.h
extern "C" int32_t lvba_balm_eval_blocks(lvba_balm_t h, const double *poses, int64_t capacity, int32_t *bi, int32_t *bj,
                                         double *blocks, int64_t *n_blocks, double *g, double *cost_avg)
{
    if (!h || !poses || !n_blocks) return fail(LVBA_ERR_ARG, "NULL argument");
    if (capacity > 0 && (!bi || !bj || !blocks)) return fail(LVBA_ERR_ARG, "NULL block arrays");
    TRY(finalize(h));
    TRY(prior_sync(h));
    TRY(loss_sync(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    // The block set is STRUCTURAL (the pair lists' destinations + the diagonal; the union pattern in a multi-rank job): it is
    // known from the set-up, the same for every call, and a sizing call (capacity 0, no g, no cost) runs no evaluation.
    lvba::hvec<int64_t> slots;
    TRY(bs_pattern_slots(bs, slots));
    const int64_t nb = (int64_t)slots.size();
    *n_blocks = nb;
    if (capacity <= 0 && !g && !cost_avg) return LVBA_OK;
    if (capacity > 0 && nb > capacity) return fail(LVBA_ERR_ARG, "capacity %lld < %lld blocks", (long long)capacity, (long long)nb);
    TRY(upload_poses(h, poses, h->d_pose_cur));
    h->lin_at_cur = false;
    TRY(enqueue_eval(h, h->d_pose_cur));
    HIPCHK(hipMemcpyAsync(h->h_pin, bs.scal(), sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    if (g) {
        launch_export_vec(bs.g(), bs.d_perm, h->N, h->d_out, bs.stream);
        HIPCHK(hipMemcpyAsync(g, h->d_out, (size_t)6 * h->N * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    }
    HIPCHK(hipStreamSynchronize(bs.stream));
    ev_collect(h);
    if (cost_avg) *cost_avg = h->h_pin[0] / (double)h->Vglobal;
    if (capacity <= 0) return LVBA_OK;
    // one device-side gather of the pattern's blocks, downloaded in slabs; then into the caller's pose order, in place
    TRY(bs_download_blocks(bs, slots.data(), nb, blocks));
    const int64_t Bb1 = (int64_t)bs.Bb + 1;
    for (int64_t q = 0; q < nb; ++q) {
        const int64_t J = slots[(size_t)q] / Bb1, dI = slots[(size_t)q] - J * Bb1;
        double *o = blocks + q * 36, b[36];
        memcpy(b, o, sizeof b); // column-major: b[c * 6 + r] = H(6 I + r, 6 J + c), I = J + dI (diagonal: r >= c only)
        const int32_t pi = bs.perm[(size_t)(J + dI)], pj = bs.perm[(size_t)J];
        if (dI == 0) {
            bi[q] = pi; bj[q] = pj;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) o[6 * r + c] = r >= c ? b[c * 6 + r] : b[r * 6 + c];
        } else if (pi >= pj) {
            bi[q] = pi; bj[q] = pj;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) o[6 * r + c] = b[c * 6 + r];
        } else { // the caller's order flips the pair: the transposed block
            bi[q] = pj; bj[q] = pi;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) o[6 * r + c] = b[r * 6 + c];
        }
    }
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_solve(lvba_balm_t h, double u, double *dx)
{
    if (!h || !dx) return fail(LVBA_ERR_ARG, "NULL argument");
    if (!h->finalized || !h->have_eval) return fail(LVBA_ERR_STATE, "lvba_balm_solve needs a prior lvba_balm_eval");
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(enqueue_solve(h, u));
    launch_export_vec(bs.d_dx, bs.d_perm, h->N, h->d_out, bs.stream);
    HIPCHK(hipMemcpyAsync(dx, h->d_out, (size_t)6 * h->N * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    int st = 0;
    HIPCHK(hipMemcpyAsync(&st, bs.d_status, sizeof(int), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    ev_collect(h);
    if (st) return fail(LVBA_NUM_FACTORIZATION, "zero or non-finite pivot in LDL^T");
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ marginal covariance
extern "C" void lvba_cov_default_opts(lvba_cov_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->anchor = -1;
    o->min_pivot_ratio = 1e-10;
}

// Sigma = H^-1 at `poses` (include/lvba_hip.h): the evaluation, the band fill with u = 0 and the anchor, a one-ended LDL^T, its pivot
// test, the selected inversion on the band of the factor and the gather (ldlt_selinv.h).  Sharded handles all-reduce H in the
// evaluation and then run the rest on their own copy: every rank computes the same bits.
extern "C" int32_t lvba_balm_covariance(lvba_balm_t h, const double *poses, const lvba_cov_opts *opts, double *diag, int64_t n_pairs,
                                        const int32_t *pi, const int32_t *pj, double *blocks, uint8_t *avail)
{
    if (!h || !poses) return fail(LVBA_ERR_ARG, "NULL argument");
    if (n_pairs < 0 || (n_pairs > 0 && (!pi || !pj || !blocks || !avail))) return fail(LVBA_ERR_ARG, "NULL pair arrays");
    lvba_cov_opts o;
    lvba_cov_default_opts(&o);
    if (opts) o = *opts;
    const int32_t N = h->N;
    if (o.anchor < -1 || o.anchor >= N) return fail(LVBA_ERR_ARG, "anchor %d out of range [-1, %d)", o.anchor, N);
    if (!(o.min_pivot_ratio >= 0.0) || !isfinite(o.min_pivot_ratio)) return fail(LVBA_ERR_ARG, "min_pivot_ratio must be finite and >= 0");
    for (int64_t k = 0; k < n_pairs; ++k)
        if (pi[k] < 0 || pi[k] >= N || pj[k] < 0 || pj[k] >= N || pi[k] == pj[k])
            return fail(LVBA_ERR_ARG, "pair %lld (%d, %d): indices out of range or equal", (long long)k, pi[k], pj[k]);
    if (h->lm_active) return fail(LVBA_ERR_STATE, "lvba_balm_covariance between lm_begin and lm_end");
    if (h->n_groups > 0) return fail(LVBA_ERR_UNSUPPORTED, "lvba_balm_covariance: grouped handles are not supported");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    if (bs.nd.active) return fail(LVBA_ERR_UNSUPPORTED, "lvba_balm_covariance: dissected handles (nd_kind != 0) are not supported");
    if (bs.d_bcr || !bs.d_A || !bs.d_work) return fail(LVBA_ERR_UNSUPPORTED, "lvba_balm_covariance: no LDL^T store on this handle");
    TRY(prior_sync(h));
    TRY(loss_sync(h));
    HIPCHK(hipSetDevice(bs.device));
    const bool timing = timing_on("cov", true);
    hipEvent_t tev[5] = {};
    if (timing)
        for (hipEvent_t &e : tev) HIPCHK(hipEventCreate(&e));
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 5; ++i) if (e[i]) hipEventDestroy(e[i]); } } evg{tev};
    auto mark = [&](int i) { if (timing) hipEventRecord(tev[i], bs.stream); };
    const int64_t n = 6 * (int64_t)N;
    LdltMat A = bs.A;
    A.no_twist = 1;
    const bool band = A.ld != n;
    const int64_t anchor_col = o.anchor >= 0 ? 6 * (int64_t)bs.iperm[(size_t)o.anchor] : -1;
    // device scratch: the selected inversion's partial products | u = 0 | pivot flag | iperm | pair indices | outputs
    const int64_t ns = ldlt_selinv_scratch_doubles(n, A.bw);
    const int64_t nout = ((int64_t)N + n_pairs) * 36;
    const int64_t nint = (int64_t)N + 2 * n_pairs + 2 * 64, nbytes8 = (n_pairs + 7) / 8 + 8;
    DevBuf scr(bs.stream); // raw scratch, carved into doubles, bytes and int32s below
    DevArr<double> zd(bs.stream);
    HIPCHK(scr.alloc((size_t)(ns + 8 + nout + nbytes8) * sizeof(double) + (size_t)nint * sizeof(int32_t)));
    double *d_sc = scr.as<double>(), *d_zero = d_sc + ns, *d_out = d_zero + 8;
    uint8_t *d_av = reinterpret_cast<uint8_t *>(d_out + nout);
    int32_t *d_i32 = reinterpret_cast<int32_t *>(d_out + nout + nbytes8);
    int *d_flag = d_i32, *d_iperm = d_i32 + 64, *d_pi = d_iperm + N + 64, *d_pj = d_pi + n_pairs;
    HIPCHK(hipMemsetAsync(d_zero, 0, 8 * sizeof(double), bs.stream)); // u = 0
    HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), bs.stream));
    HIPCHK(hipMemcpyAsync(d_iperm, bs.iperm.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, bs.stream));
    if (n_pairs > 0) {
        HIPCHK(hipMemcpyAsync(d_pi, pi, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, bs.stream));
        HIPCHK(hipMemcpyAsync(d_pj, pj, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, bs.stream));
    }
    // Z: the second-matrix slot of the band store (unused by a one-ended factorisation); its own buffer for dense storage
    double *z = nullptr;
    const LdltSelinvRoom sroom{bs.room.store, band ? ldlt_store_room(bs.room.store, n, A.ld, true) : ldlt_cov_z_dense_doubles(n), bs.room.work, ns};
    if (band) z = bs.d_A + ldlt_mat2_offset(n, A.ld);
    else {
        HIPCHK(zd.alloc((size_t)sroom.z));
        z = zd;
    }
    // the band store must read as zero outside what the damped solve rewrites (block_system.hip): zeroed again on every way out
    const size_t band_bytes = band ? (size_t)bs.room.store * sizeof(double) : 0;
    struct BandGuard { double *p; size_t b; hipStream_t s; ~BandGuard() { if (p) (void)hipMemsetAsync(p, 0, b, s); } } bandg{band ? bs.d_A : nullptr, band_bytes, bs.stream};
    mark(0);
    TRY(upload_poses(h, poses, h->d_pose_cur));
    h->lin_at_cur = false;
    TRY(enqueue_eval(h, h->d_pose_cur));
    h->have_eval = false; // the solver's workspace now holds the covariance's factor: a later solve needs a fresh evaluation
    mark(1);
    TRY(ldlt_solve(A, bs.Hblk(), bs.Bb, N, bs.g(), d_zero, bs.d_dx, bs.d_work, bs.room, bs.d_status, bs.stream, nullptr, nullptr, LDLT_FACTOR,
                   nullptr, anchor_col));
    ldlt_cov_pivot_check(A, bs.Hblk(), bs.Bb, bs.d_work, anchor_col, o.min_pivot_ratio, bs.d_status, d_flag, bs.stream);
    mark(2);
    int *h_flag = reinterpret_cast<int *>(h->h_pin);
    HIPCHK(hipMemcpyAsync(h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(bs.stream));
    ev_collect(h);
    if (*h_flag) return fail(LVBA_NUM_FACTORIZATION, "lvba_balm_covariance: H is not positive definite at these poses (pivot test "
                                                     "failed; no anchor and no priors that fix the frame, or not at a minimum)");
    mark(3);
    TRY(ldlt_selinv(A, z, bs.d_work, d_sc, sroom, bs.stream));
    mark(4);
    ldlt_cov_gather(z, A.ld, band ? bs.Bb : -1, d_iperm, N, o.anchor, n_pairs, d_pi, d_pj, d_out, d_out + (int64_t)N * 36, d_av, bs.stream);
    HIPCHK(hipGetLastError());
    if (diag) HIPCHK(hipMemcpyAsync(diag, d_out, (size_t)N * 36 * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    if (n_pairs > 0) {
        HIPCHK(hipMemcpyAsync(blocks, d_out + (int64_t)N * 36, (size_t)n_pairs * 36 * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
        HIPCHK(hipMemcpyAsync(avail, d_av, (size_t)n_pairs, hipMemcpyDeviceToHost, bs.stream));
    }
    HIPCHK(hipStreamSynchronize(bs.stream));
    if (timing) {
        // (the gather's time includes the download of the blocks)
        hipEvent_t e5 = nullptr;
        HIPCHK(hipEventCreate(&e5));
        hipEventRecord(e5, bs.stream);
        hipEventSynchronize(e5);
        float t[4] = {};
        hipEventElapsedTime(&t[0], tev[0], tev[1]);
        hipEventElapsedTime(&t[1], tev[1], tev[2]);
        hipEventElapsedTime(&t[2], tev[3], tev[4]);
        hipEventElapsedTime(&t[3], tev[4], e5);
        hipEventDestroy(e5);
        fprintf(stderr, "lvba cov: eval %.3f ms factor %.3f ms selinv %.3f ms gather %.3f ms (n %lld, bw %lld, %s)\n", t[0], t[1], t[2],
                t[3], (long long)n, (long long)A.bw, band ? "band" : "dense");
    }
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ a8: LM
extern "C" int32_t lvba_balm_lm_begin(lvba_balm_t h, const double *poses, const lvba_balm_opts *opts)
{
    if (!h || !poses) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    TRY(prior_sync(h));
    TRY(loss_sync(h));
    HIPCHK(hipSetDevice(h->bs.device));
    if (opts) h->lm_opts = *opts; else lvba_balm_default_opts(&h->lm_opts);
    if (h->lm_opts.max_iter < 0) return fail(LVBA_ERR_ARG, "max_iter < 0");
    TRY(upload_poses(h, poses, h->d_pose_cur));
    h->lm.begin(h->lm_opts.u0, h->lm_opts.v0, h->lm_opts.max_iter);
    h->residual1 = 0.0;
    h->lin_at_cur = false;
    h->lm_active = true;
    return LVBA_OK;
}

// One trip through bavoxel.hpp:686-766.
extern "C" int32_t lvba_balm_lm_step(lvba_balm_t h, lvba_lm_trace *row, int32_t *done)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    if (!h->lm_active) return fail(LVBA_ERR_STATE, "lm_step without lm_begin");
    LmRule &lm = h->lm;
    if (lm.done) { if (done) *done = 1; return fail(LVBA_ERR_STATE, "LM loop already finished"); }
    HIPCHK(hipSetDevice(h->bs.device));
    const bool evaluated = lm.evaluate;
    // The trial point is costed by the VOXEL PASS of the evaluation (cost + voxel records): an accepted trial point is where the
    // next evaluation happens, and that evaluation then starts from the records (factor pass, pair pass) instead of reading
    // and eigen-decomposing every voxel again.  A rejected step wastes the difference to the cost-only kernel (C3: 0.04 ms).
    // Also on voxel shards (the records are local).
    if (evaluated) TRY(enqueue_eval(h, h->d_pose_cur, h->lin_at_cur));                     // :688-689
    TRY(enqueue_solve(h, lm.u));                                                           // :692-710
    const int n_q1 = launch_retract_q1(h->d_pose_cur, h->bs.d_dx, h->d_pose_trial, h->N, h->bs.Hblk(), h->bs.Bb, h->bs.g(), lm.u, h->d_q1part,
                                       h->stream());                                       // :722-729 (retraction + the q1 numerator's shares)
    TRY(enqueue_cost(h, h->d_pose_trial, h->d_scal2, true));                               // :731 (+ the linearisation at the trial point)
    h->lin_at_cur = false; // it belongs to the trial point now
    launch_lm_report(h->d_scal2, h->d_q1part, n_q1, h->bs.scal(), h->bs.d_status, h->h_pin, h->stream()); // -> pinned host memory, zero-copy
    HIPCHK(hipStreamSynchronize(h->stream()));
    ev_collect(h);
    const double Vg = (double)h->Vglobal;
    if (evaluated) h->residual1 = h->h_pin[2] / Vg;                                        // AVG_THR :634-635
    long long st = 0;
    memcpy(&st, h->h_pin + 4, sizeof st);
    // :732-760, the costs averaged over the voxels; a flagged solve counts as a rejected step whatever the kernels left in dx
    const lvba_lm_trace r = lm.step(h->residual1, h->h_pin[0] / Vg, h->h_pin[1] / Vg, (int)st != 0, h->lm_opts.rel_tol, h->lm_opts.max_iter, true);
    if (row) *row = r;
    if (r.accepted) {
        std::swap(h->d_pose_cur, h->d_pose_trial);
        h->lin_at_cur = true; // the trial point is the current point now
    }
    if (done) *done = lm.done ? 1 : 0;
    // numerical statuses (> 0) are reported, not fatal: the caller may keep stepping, as BALM2::damping_iter does
    if (r.status == LVBA_NUM_FACTORIZATION) return fail(r.status, "zero or non-finite pivot in LDL^T (iteration %d)", r.iter);
    if (r.status == LVBA_NUM_NONFINITE) return fail(r.status, "non-finite cost (iteration %d)", r.iter);
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_lm_end(lvba_balm_t h, double *poses_out)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    if (!h->lm_active) return fail(LVBA_ERR_STATE, "lm_end without lm_begin");
    HIPCHK(hipSetDevice(h->bs.device));
    if (poses_out) {
        TRY(download_poses(h, h->d_pose_cur, poses_out));
    }
    h->lm_active = false;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_refine(lvba_balm_t h, double *poses_inout, const lvba_balm_opts *opts,
                                    lvba_lm_trace *trace, int32_t *n_trace)
{
    if (!h || !poses_inout) return fail(LVBA_ERR_ARG, "NULL argument");
    if (n_trace) *n_trace = 0;
    TRY(lvba_balm_lm_begin(h, poses_inout, opts));
    int32_t rows = 0, done = h->lm.done ? 1 : 0, rc = LVBA_OK, worst = LVBA_OK;
    char worst_msg[512] = "";
    while (!done) {
        lvba_lm_trace row;
        rc = lvba_balm_lm_step(h, &row, &done);
        if (rc < 0) break;
        if (trace) trace[rows] = row;
        rows++;
        // a numerical failure (zero pivot, non-finite cost) does NOT end the loop: BALM2::damping_iter (bavoxel.hpp:686-766)
        // has no such exit -- the step is rejected, u *= v, and up to 10 iterations run.  The status is kept in the trace row
        // and the worst one is returned at the end.
        if (rc > worst) { worst = rc; snprintf(worst_msg, sizeof worst_msg, "%s", lvba_last_error()); }
    }
    if (n_trace) *n_trace = rows;
    const int32_t rc2 = lvba_balm_lm_end(h, poses_inout);
    if (rc < 0) return rc;
    if (rc2 != LVBA_OK) return rc2;
    if (worst != LVBA_OK) return fail(worst, "%s", worst_msg);
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ grouped LM
// Several INDEPENDENT problems in one handle: group k owns the poses [pose_off[k], pose_off[k+1]) and the voxels
// [voxel_off[k], voxel_off[k+1]), and every factor of its voxels is seen from one of its poses -- the windows of
// LvbaSystem::runWindowBA (src/lvba_system.cpp:232-302), which the reference optimises one after the other.  The Hessian is
// block diagonal, so ONE evaluation, ONE band factorisation (damping per group) and ONE cost pass serve all groups per LM
// iteration; every group keeps the LM state of BALM2::damping_iter (bavoxel.hpp:662-767) for itself.
extern "C" int32_t lvba_balm_set_groups(lvba_balm_t h, int32_t n_groups, const int32_t *pose_off, const int64_t *voxel_off)
{
    if (!h || !pose_off || !voxel_off) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->finalized) return fail(LVBA_ERR_STATE, "set_groups must precede the first cost/eval/refine call");
    if (h->bs.distributed()) return fail(LVBA_ERR_UNSUPPORTED, "groups and voxel shards do not combine");
    if (!h->priors.empty()) return fail(LVBA_ERR_STATE, "a handle with pose priors cannot be grouped");
    if (n_groups < 1) return fail(LVBA_ERR_ARG, "n_groups must be >= 1");
    if (pose_off[0] != 0 || pose_off[n_groups] != h->N || voxel_off[0] != 0 || voxel_off[n_groups] != h->V)
        return fail(LVBA_ERR_ARG, "the groups must cover all poses and all voxels");
    for (int32_t k = 0; k < n_groups; ++k) {
        if (pose_off[k + 1] <= pose_off[k] || voxel_off[k + 1] <= voxel_off[k]) return fail(LVBA_ERR_ARG, "group %d is empty", k);
        for (int64_t f = h->h_voff[voxel_off[k]]; f < h->h_voff[voxel_off[k + 1]]; ++f)
            if (h->h_pidx[f] < pose_off[k] || h->h_pidx[f] >= pose_off[k + 1])
                return fail(LVBA_ERR_ARG, "a voxel of group %d is seen from pose %d, which belongs to another group", k, h->h_pidx[f]);
    }
    HIPCHK(hipSetDevice(h->bs.device));
    BlockSys &bs = h->bs;
    // chunks must not straddle groups: the chunk table is made again with breaks at the group boundaries
    lvba::hvec<int64_t> chunk_v0;
    int64_t Q = 0;
    if (lvba::chunk_voxels(h->V, h->h_voff.data(), LVBA_CF, LVBA_CV, chunk_v0, Q, voxel_off + 1, n_groups - 1) >= 0)
        return fail(LVBA_ERR_STATE, "chunk table");
    lvba::DevicePool::get().free(h->d_chunk_v0); bs.device_bytes -= (h->n_chunks + 1) * (int64_t)sizeof(int64_t); h->d_chunk_v0 = nullptr;
    lvba::DevicePool::get().free(h->d_chunk_cost); bs.device_bytes -= h->n_chunks * (int64_t)sizeof(double); h->d_chunk_cost = nullptr;
    h->n_chunks = (int64_t)chunk_v0.size() - 1;
    TRY(bs_dmalloc(bs, &h->d_chunk_v0, h->n_chunks + 1));
    TRY(bs_dmalloc(bs, &h->d_chunk_cost, h->n_chunks));
    HIPCHK(lvba::copy_h2d(h->d_chunk_v0, chunk_v0.data(), (size_t)(h->n_chunks + 1) * sizeof(int64_t)));
    lvba::hvec<int64_t> gco((size_t)n_groups + 1, 0);
    {
        int64_t c = 0;
        for (int32_t k = 0; k <= n_groups; ++k) {
            while (c < h->n_chunks && chunk_v0[(size_t)c] < voxel_off[k]) ++c;
            if (chunk_v0[(size_t)c] != voxel_off[k]) return fail(LVBA_ERR_STATE, "group %d does not start on a chunk", k);
            gco[(size_t)k] = c;
        }
    }
    lvba::hvec<int32_t> gof((size_t)h->N);
    for (int32_t k = 0; k < n_groups; ++k)
        for (int32_t j = pose_off[k]; j < pose_off[k + 1]; ++j) gof[(size_t)j] = k;
    h->n_groups = n_groups;
    {
        int32_t span = 0; // block half-bandwidth in the caller's pose order: no voxel leaves its group (checked above)
        for (int32_t k = 0; k < n_groups; ++k) span = std::max(span, pose_off[k + 1] - pose_off[k] - 1);
        bs.bb_hint = span;
    }
    h->g_pose_off.assign(pose_off, pose_off + n_groups + 1);
    h->g_vox_off.assign(voxel_off, voxel_off + n_groups + 1);
    TRY(bs_dmalloc(bs, &h->d_grp_of_pose, h->N));
    TRY(bs_dmalloc(bs, &h->d_gpo, n_groups + 1));
    TRY(bs_dmalloc(bs, &h->d_gaccept, n_groups));
    TRY(bs_dmalloc(bs, &h->d_gco, n_groups + 1));
    TRY(bs_dmalloc(bs, &h->d_gscal, 3 * (int64_t)n_groups));
    HIPCHK(lvba::copy_h2d(h->d_grp_of_pose, gof.data(), (size_t)h->N * sizeof(int32_t)));
    HIPCHK(lvba::copy_h2d(h->d_gpo, pose_off, (size_t)(n_groups + 1) * sizeof(int32_t)));
    HIPCHK(lvba::copy_h2d(h->d_gco, gco.data(), (size_t)(n_groups + 1) * sizeof(int64_t)));
    HIPCHK(lvba::PinnedCache::get().acquire((void **)&h->h_gpin, std::max<size_t>(4096, 3 * (size_t)n_groups * sizeof(double))));
    HIPCHK(lvba::PinnedCache::get().acquire((void **)&h->h_gacc, std::max<size_t>(4096, (size_t)n_groups * sizeof(int32_t))));
    // the caller's pose order is the solver's: the block-diagonal structure stays, and pose -> group is a plain table
    bs.ordering = 0;
    bs.n_groups = n_groups;
    bs.d_grp_of_pose = h->d_grp_of_pose;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_refine_groups(lvba_balm_t h, double *poses_inout, const lvba_balm_opts *opts, int32_t *n_iter,
                                           int32_t *status, double *cost_first, double *cost_last)
{
    if (!h || !poses_inout) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->n_groups < 1) return fail(LVBA_ERR_STATE, "refine_groups without set_groups");
    TRY(finalize(h));
    if (h->bs.d_bcr) return fail(LVBA_ERR_UNSUPPORTED, "grouped refinement needs the LDL^T solver");
    HIPCHK(hipSetDevice(h->bs.device));
    lvba_balm_opts o;
    if (opts) o = *opts; else lvba_balm_default_opts(&o);
    if (o.max_iter < 0) return fail(LVBA_ERR_ARG, "max_iter < 0");
    const int32_t G = h->n_groups;
    BlockSys &bs = h->bs;
    hipStream_t s = h->stream();
    TRY(upload_poses(h, poses_inout, h->d_pose_cur));
    struct St { LmRule lm; double r1; int32_t status; double first, last; };
    lvba::hvec<St> st((size_t)G);
    for (auto &q : st) {
        q = St{LmRule{}, 0.0, LVBA_OK, 0.0, 0.0};
        q.lm.begin(o.u0, o.v0, o.max_iter);
    }
    lvba::hvec<double> u((size_t)G);
    double *c1 = h->d_gscal, *c2 = h->d_gscal + G, *q1d = h->d_gscal + 2 * (int64_t)G;
    int32_t worst = LVBA_OK;
    for (;;) {
        bool any = false, need_eval = false;
        for (const auto &q : st) { any = any || !q.lm.done; need_eval = need_eval || (!q.lm.done && q.lm.evaluate); }
        if (!any) break;
        if (need_eval) { // :688-689 (groups whose last step was rejected get the same H, g, cost again: the kernels are deterministic)
            TRY(enqueue_eval(h, h->d_pose_cur));
            launch_reduce_chunks_groups(h->d_chunk_cost, h->d_gco, G, c1, s);
        }
        // finished groups stay in the joint system as identity blocks (negative damping: ldlt_prepare_kernel): they cost
        // nothing to factorise and cannot raise the pivot flag for the groups that are still running
        for (int32_t k = 0; k < G; ++k) u[(size_t)k] = st[(size_t)k].lm.done ? -1.0 : st[(size_t)k].lm.u;
        ev_begin(h, EV_SOLVE);
        TRY(bs_enqueue_solve_groups(bs, u.data()));                                            // :692-710
        ev_end(h, EV_SOLVE);
        launch_retract(h->d_pose_cur, bs.d_dx, h->d_pose_trial, h->N, s);                      // :722-727
        launch_predicted_decrease_groups(bs.Hblk(), bs.Bb, bs.g(), bs.d_dx, bs.d_u, h->d_gpo, G, q1d, s); // :729
        launch_cost_chunks(h->dev(), h->d_pose_trial, h->d_chunk_cost, s);                     // :731
        launch_reduce_chunks_groups(h->d_chunk_cost, h->d_gco, G, c2, s);
        HIPCHK(hipMemcpyAsync(h->h_gpin, h->d_gscal, 3 * (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h->h_pin + 4, bs.d_status, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ev_collect(h);
        int pivot = 0;
        memcpy(&pivot, h->h_pin + 4, sizeof(int));
        // a zero pivot in one group's block poisons the band below it: the groups are not independent any more
        if (pivot) return fail(LVBA_NUM_FACTORIZATION, "zero or non-finite pivot in LDL^T of the grouped system");
        for (int32_t k = 0; k < G; ++k) {
            St &q = st[(size_t)k];
            h->h_gacc[k] = 0;
            if (q.lm.done) continue;
            const double Vg = (double)(h->g_vox_off[(size_t)k + 1] - h->g_vox_off[(size_t)k]);
            if (need_eval && q.lm.evaluate) q.r1 = h->h_gpin[k] / Vg;                          // AVG_THR :634-635
            if (q.lm.iter == 0) q.first = q.r1;
            // :732-760, the costs averaged over the group's voxels
            const lvba_lm_trace r = q.lm.step(q.r1, h->h_gpin[G + k] / Vg, h->h_gpin[2 * G + k] / Vg, false, o.rel_tol, o.max_iter, true);
            h->h_gacc[k] = r.accepted;
            q.last = r.accepted ? r.residual2 : r.residual1;
            if (r.status > q.status) q.status = r.status;
            if (q.status > worst) worst = q.status;
        }
        HIPCHK(hipMemcpyAsync(h->d_gaccept, h->h_gacc, (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, s));
        launch_select_poses(h->d_pose_cur, h->d_pose_trial, h->d_gaccept, h->d_grp_of_pose, h->N, s);
        HIPCHK(hipStreamSynchronize(s)); // h_gacc is rewritten in the next iteration
    }
    TRY(download_poses(h, h->d_pose_cur, poses_inout));
    for (int32_t k = 0; k < G; ++k) {
        if (n_iter) n_iter[k] = st[(size_t)k].lm.iter;
        if (status) status[k] = st[(size_t)k].status;
        if (cost_first) cost_first[k] = st[(size_t)k].first;
        if (cost_last) cost_last[k] = st[(size_t)k].last;
    }
    if (worst != LVBA_OK) return fail(worst, "non-finite cost in a group");
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ pose priors
// The model is in prior_device.h, the passes in priors.hip.  A prior adds its terms to the store after the voxel evaluation (and
// after its all-reduce: every rank adds them once, to the same reduced buffer, so the ranks stay bitwise equal).
// the blocks the voxel evaluation writes (diagonal included): a prior adds to those and writes the others, which hold nothing else
static int32_t prior_vox_slots(lvba_balm_s *h)
{
    if (h->vox_slots_known) return LVBA_OK;
    BlockSys &bs = h->bs;
    h->vox_all_add = bs.distributed() && !bs.d_ar_slot; // a multi-rank job without a union pattern clears the whole store
    lvba::hvec<int64_t> keep;
    keep.swap(bs.extra_slots);
    const int32_t rc = h->vox_all_add ? LVBA_OK : bs_pattern_slots(bs, h->vox_slots);
    keep.swap(bs.extra_slots);
    TRY(rc);
    h->vox_slots_known = true;
    return LVBA_OK;
}

// h->priors -> the solver order, the scatter tables and their device copies (the handle is finalised)
static int32_t bind_priors(lvba_balm_s *h)
{
    BlockSys &bs = h->bs;
    TRY(h->pt.release(bs));
    bs.extra_slots.clear();
    if (h->priors.empty()) return LVBA_OK;
    TRY(prior_vox_slots(h));
    return h->pt.bind(bs, h->priors, h->vox_slots, h->vox_all_add, 1, &bs.extra_slots);
}

// Sharded handles: the first collective call after lvba_balm_set_priors (or the set-up) checks with one MAX all-reduce of
// (count, hash) and their negations that every rank holds the same priors (reserved fields are stored as zero).
static int32_t prior_sync(lvba_balm_s *h)
{
    if (!h->prior_check) return LVBA_OK;
    BlockSys &bs = h->bs;
    if (bs.distributed()) {
        const int64_t v[2] = {(int64_t)h->priors.size(), prior_hash(h->priors)};
        bool same[2];
        HIPCHK(hipSetDevice(bs.device));
        TRY(bs_ranks_agree(bs, v, 2, same));
        if (!same[0] || !same[1]) return fail(LVBA_ERR_ARG, "the ranks of this job set different pose priors");
    }
    h->prior_check = false;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_set_priors(lvba_balm_t h, int32_t n, const lvba_prior *priors)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    if (n < 0 || (n > 0 && !priors)) return fail(LVBA_ERR_ARG, "n must be >= 0 and priors non-NULL");
    TRY(prior_cap(n));
    if (n > 0 && h->n_groups > 0) return fail(LVBA_ERR_STATE, "a grouped handle (lvba_balm_set_groups) takes no pose priors");
    if (h->lm_active) return fail(LVBA_ERR_STATE, "set_priors between lvba_balm_lm_begin and lvba_balm_lm_end");
    TRY(prior_validate(n, priors, h->N));
    BlockSys &bs = h->bs;
    if (h->finalized) { // the store is laid out: every relative pair must be one of its blocks
        const bool nd = bs.nd.active; // a dissected system couples only the pairs its plan was made from
        if (nd && n > 0) TRY(prior_vox_slots(h));
        TRY(prior_pairs_in_store(bs, n, priors, nd ? &h->vox_slots : nullptr, nd ? &h->build_slots : nullptr, "poses", "eval"));
    }
    prior_store(bs, h->finalized, n, priors, h->priors);
    h->prior_check = true;
    return h->finalized ? bind_priors(h) : LVBA_OK;
}

extern "C" int32_t lvba_balm_prior_residuals(lvba_balm_t h, const double *poses, double *e, double *cost)
{
    if (!h || !poses) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    const int64_t n = h->pt.dev.n;
    if (n == 0) { if (cost) *cost = 0.0; return LVBA_OK; }
    TRY(upload_poses(h, poses, h->d_pose_trial));
    DevArr<double> d(bs.stream);
    HIPCHK(d.alloc((size_t)(6 * n + 1)));
    double *de = d;
    HIPCHK(hipMemsetAsync(de + 6 * n, 0, sizeof(double), bs.stream));
    launch_prior_cost(h->pt.dev, h->d_pose_trial, de + 6 * n, de, bs.stream);
    HIPCHK(hipGetLastError());
    double c = 0.0;
    if (e) HIPCHK(hipMemcpyAsync(e, de, (size_t)(6 * n) * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipMemcpyAsync(&c, de + 6 * n, sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    if (cost) *cost = c;
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ robust loss
// C(x) = sum_v rho(lambda_min(v)) + priors; g = sum_v rho' g_v, H = sum_v rho' H_v (the rho'' g_v g_v^T term is left out, see
// include/lvba_hip.h).  The loss lives on the handle and reaches the kernels through BalmDev (dev()): the voxel pass turns lambda_min
// into rho and leaves rho' in the voxel record, the factor pass scales with it; nothing else in the LM loop knows about it.
namespace lvba {
int32_t loss_validate(const lvba_loss *loss, const char *what)
{
    if (!loss || loss->kind == LVBA_LOSS_TRIVIAL) return LVBA_OK;
    if (loss->kind < LVBA_LOSS_TRIVIAL || loss->kind > LVBA_LOSS_TUKEY) return fail(LVBA_ERR_ARG, "%s: unknown loss kind %d", what, loss->kind);
    if (!isfinite(loss->scale) || !(loss->scale > 0.0)) return fail(LVBA_ERR_ARG, "%s: the loss scale must be finite and > 0", what);
    return LVBA_OK;
}
} // namespace lvba

extern "C" int32_t lvba_balm_set_loss(lvba_balm_t h, const lvba_loss *loss)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    TRY(lvba::loss_validate(loss, "lvba_balm_set_loss"));
    if (h->lm_active) return fail(LVBA_ERR_STATE, "set_loss between lvba_balm_lm_begin and lvba_balm_lm_end");
    if (!loss || loss->kind == LVBA_LOSS_TRIVIAL) h->loss = lvba_loss{LVBA_LOSS_TRIVIAL, 0, 0.0};
    else h->loss = lvba_loss{loss->kind, 0, loss->scale};
    h->loss_check = true;
    h->have_eval = false; // H, g and the voxel records belong to the old cost
    h->lin_at_cur = false;
    return LVBA_OK;
}

// Sharded handles: like prior_sync, one MAX all-reduce of (kind, scale bits) and their negations
static int32_t loss_sync(lvba_balm_s *h)
{
    if (!h->loss_check) return LVBA_OK;
    BlockSys &bs = h->bs;
    if (bs.distributed()) {
        int64_t v[2] = {h->loss.kind, 0};
        memcpy(&v[1], &h->loss.scale, sizeof v[1]); // (a valid scale is >= 0: the sign bit is clear)
        bool same[2];
        HIPCHK(hipSetDevice(bs.device));
        TRY(bs_ranks_agree(bs, v, 2, same));
        if (!same[0] || !same[1]) return fail(LVBA_ERR_ARG, "the ranks of this job set different losses (lvba_balm_set_loss)");
    }
    h->loss_check = false;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_voxel_residuals(lvba_balm_t h, const double *poses, double *lambda_min, double *weight)
{
    if (!h || !poses) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    if (!lambda_min && !weight) return LVBA_OK;
    TRY(upload_poses(h, poses, h->d_pose_trial));
    const int64_t V = h->V;
    DevArr<double> d(bs.stream);
    HIPCHK(d.alloc((size_t)((lambda_min ? V : 0) + (weight ? V : 0))));
    double *dl = d, *dw = dl + (lambda_min ? V : 0);
    launch_voxel_residuals(h->dev(), h->d_pose_trial, h->d_vox_order, lambda_min ? dl : nullptr, weight ? dw : nullptr, bs.stream);
    HIPCHK(hipGetLastError());
    if (lambda_min) HIPCHK(hipMemcpyAsync(lambda_min, dl, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    if (weight) HIPCHK(hipMemcpyAsync(weight, dw, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ multi-GPU
extern "C" int32_t lvba_balm_dist_init(lvba_balm_t h, int32_t n_ranks, int32_t rank, const char uid[128])
{
    if (!h || !uid) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->finalized) return fail(LVBA_ERR_STATE, "dist_init must precede the first cost/eval/refine call");
    if (h->n_groups > 0) return fail(LVBA_ERR_UNSUPPORTED, "groups and voxel shards do not combine");
    int64_t Vg = h->V;
    TRY(bs_dist_init(h->bs, n_ranks, rank, uid, &Vg));
    h->Vglobal = Vg;
    return LVBA_OK;
}

extern "C" int32_t lvba_balm_dist_init_external(lvba_balm_t h, int32_t n_ranks, int32_t rank, lvba_allreduce_fn fn, void *ctx)
{
    if (!h || !fn) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->finalized) return fail(LVBA_ERR_STATE, "dist_init must precede the first cost/eval/refine call");
    if (h->n_groups > 0) return fail(LVBA_ERR_UNSUPPORTED, "groups and voxel shards do not combine");
    int64_t Vg = h->V;
    TRY(bs_dist_init_external(h->bs, n_ranks, rank, fn, ctx, &Vg));
    h->Vglobal = Vg;
    return LVBA_OK;
}
