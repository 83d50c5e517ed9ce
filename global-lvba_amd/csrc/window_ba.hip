// window_ba.hip -- the window-BA stage that turns raw scans + odometry into anchor frames, on the device.
//
// Replaces LvbaSystem::runWindowBA (reference src/lvba_system.cpp:204-310): per window of `window_size` frames
//   cut_voxel / recut / tras_opt at the odometry poses   :247-257   -> lvba_voxmap_build_scans + lvba_voxmap_to_balm
//   skip if fewer than 3 plane voxels per frame           :258-262
//   BALM2::damping_iter                                   :264       -> lvba_balm_refine
//   re-alignment to the odometry pose of the first frame  :268-279   (12-double algebra, host)
//   relative poses to the anchor, merge of the clouds     :284-299   -> wba_merge_kernel (fp32 write-back as pl_transform,
//                                                                       include/BALM/tools.hpp:385-395)
//   down_sampling_voxel2                                  tools.hpp:300-359 -> key + stable sort + first-minimum per voxel
// The raw clouds never leave HBM between the stages; the anchor clouds are born there (a new lvba_scans_t) and feed the
// global stages' lvba_voxmap_build_scans directly.
// down_sampling_voxel2 emits survivors in unordered_map order (unspecified); here: sorted by voxel key (x, y, z).
#include <atomic>
#include <string>
#include <thread>
#include "host_arena.h"
#include "voxel_internal.h"
#include "lvba_internal.h"
#include "block_system.h"

using namespace lvba;

namespace {

// merged cloud of one window: every point moved into the anchor frame with its frame's relative pose and rounded to fp32
// (pl_transform); plus the leaf-voxel key and squared distance to the voxel centre of down_sampling_voxel2.
__global__ void wba_merge_kernel(int64_t P, const float *__restrict__ pts, const int64_t *__restrict__ frame_off, int n_frames,
                                 const double *__restrict__ rel, double leaf, float *__restrict__ out,
                                 uint64_t *__restrict__ key, double *__restrict__ d2, uint32_t *__restrict__ idx,
                                 int *__restrict__ err, int *__restrict__ range_partial /* voxel_internal.h: key_range_update */)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kb[3] = {0, 0, 0};
    if (i < P) {
    float q[3];
    pose_apply_f32(rel + 12 * (int64_t)frame_of_point(frame_off, n_frames, i), pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], q);
    out[3 * i] = q[0]; out[3 * i + 1] = q[1]; out[3 * i + 2] = q[2];
    if (key) {
    int64_t k[3];
    double dd;
    if (!leaf_key_of(q, leaf, k, dd)) *err = 1;
    key[i] = pack_key(k);
    d2[i] = dd;
    idx[i] = (uint32_t)i;
#pragma unroll
    for (int j = 0; j < 3; ++j) kb[j] = (int)(k[j] + KEY_BIAS);
    }
    }
    if (key) key_range_update(range_partial, kb, i < P); // (the sort runs on the bits that vary)
}
// after the stable sort by key (K: the re-packed keys, equal exactly where the leaf keys are): the run leader picks the first
// minimum of d2 in merged order
template <class K>
__global__ void wba_pick_kernel(int64_t P, const K *__restrict__ key_s, const uint32_t *__restrict__ order,
                                const double *__restrict__ d2, uint32_t *__restrict__ flag, uint32_t *__restrict__ pick)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const bool head = i == 0 || key_s[i] != key_s[i - 1];
    flag[i] = head ? 1u : 0u;
    if (!head) return;
    const K k = key_s[i];
    uint32_t best = order[i];
    double bd = d2[best];
    for (int64_t j = i + 1; j < P && key_s[j] == k; ++j) {
        const uint32_t c = order[j];
        const double d = d2[c];
        if (d < bd) { bd = d; best = c; }
    }
    pick[i] = best;
}
__global__ void wba_compact_kernel(int64_t P, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                   const uint32_t *__restrict__ pick, const float *__restrict__ merged, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P || !flag[i]) return;
    const uint32_t s = pick[i], o = excl[i];
    out[3 * (int64_t)o] = merged[3 * (int64_t)s];
    out[3 * (int64_t)o + 1] = merged[3 * (int64_t)s + 1];
    out[3 * (int64_t)o + 2] = merged[3 * (int64_t)s + 2];
}

// joint form of the merge stage (all windows in one pass): (code of the point's window << total) | re-packed leaf key -- the
// points of a window stay together, inside it the order is the leaf key's, as in the window's own sort.  code[window]: its rank
// among the windows that produce an anchor cloud; the others' points get the code above all of those and sort to the end.
template <class K>
__global__ void wba_compress_win_kernel(int64_t P, const uint64_t *key, const int64_t *__restrict__ frame_off, int n_frames, int ws,
                                        const uint32_t *__restrict__ code, const KeyPack kp, K *out /* may be key */)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint64_t c = code[frame_of_point(frame_off, n_frames, i) / ws];
    out[i] = (K)((c << kp.total) | key_compress<uint64_t>(key[i], kp)); // (in 64 bits, narrowed afterwards: key_pack.h)
}
// anchor points of every window: the scan of the leader flags read at the windows' bounds in the sorted sequence
__global__ void wba_bounds_kernel(int n, const int64_t *__restrict__ at, const uint32_t *__restrict__ excl, uint32_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = excl[at[i]];
}

inline void mat3_mul(const double *A, const double *B, double *C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
inline void mat3_mulT(const double *A, const double *B, double *C) // A * B^T
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
inline void mat3T_mul(const double *A, const double *B, double *C) // A^T * B
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}

// damping_iter on the problem of a voxel map, which it consumes (:264, :386): poses x refined in place; the LM status, the
// iterations, the first and last cost of the trace, and the time of the problem's set-up
struct Refined { int32_t status = 0, n_iter = 0; double cost_first = 0.0, cost_last = 0.0, setup_ms = 0.0; };
// loss: the robust loss of the problem's voxel costs (lvba_balm_set_loss), NULL: none
int32_t refine_map(lvba_voxmap_t map, double *x, const lvba_balm_opts &lm, Refined &r, int32_t n_priors = 0,
                   const lvba_prior *priors = nullptr, const lvba_loss *loss = nullptr)
{
    const double t0 = now_ms();
    lvba_balm_t b = nullptr;
    int32_t rc = lvba_voxmap_to_balm(map, &b);
    lvba_voxmap_destroy(map);
    if (rc != LVBA_OK) return rc;
    if (n_priors > 0 && (rc = lvba_balm_set_priors(b, n_priors, priors)) != LVBA_OK) {
        lvba_balm_destroy(b);
        return rc;
    }
    if (loss && (rc = lvba_balm_set_loss(b, loss)) != LVBA_OK) {
        lvba_balm_destroy(b);
        return rc;
    }
    lvba::hvec<lvba_lm_trace> trace((size_t)std::max(1, lm.max_iter));
    int32_t nt = 0;
    lvba_balm_info_t bi;
    lvba_balm_info(b, &bi); // forces the one-off problem set-up (ordering, pair lists) so that it is timed apart
    r.setup_ms = now_ms() - t0;
    rc = lvba_balm_refine(b, x, &lm, trace.data(), &nt);
    lvba_balm_destroy(b);
    if (rc < 0) return rc;
    r.status = rc; r.n_iter = nt;
    if (nt > 0) {
        r.cost_first = trace[0].residual1;
        r.cost_last = trace[nt - 1].accepted ? trace[nt - 1].residual2 : trace[nt - 1].residual1;
    }
    return LVBA_OK;
}

// ---- lvba_window_ba.  One window = map -> problem -> LM -> anchor cloud; windows are independent (src/lvba_system.cpp:232-302
// runs them one after the other).  The stages, each over all windows:
//   1. voxel map of every window: ONE map of all windows (stage_map_joint), or one per window on a few host threads, each with
//      its own stream (a single map build leaves the GPU idle most of the time -- launch and synchronisation latency);
//   2. the LM refinements of ALL windows in lock-step as one grouped problem (lvba_balm_set_groups / lvba_balm_refine_groups: one
//      evaluation, one band factorisation with a damping value per window, one cost pass per iteration for all windows; every
//      window keeps its own LM state).  lm_mode = 1, a single window, or a broken pivot in the joint factorisation: one window at
//      a time, on the host threads;
//   3. alignment, relative poses, anchor merge + down-sampling: all windows in one pass (merge_run over all windows), or one
//      pass per window on the host threads.
// The results are assembled in window order into the caller's arrays and a scan set of the anchor clouds.
struct WinResult {
    int32_t rc = LVBA_OK;
    std::string err;
    lvba_window_info info{};
    lvba::hvec<double> x; // the window's poses: odometry, refined by stage 2
    lvba_voxmap_t map = nullptr;
    bool refined = false;
};
// one lvba_window_ba call; it owns what the stages make until the call returns and frees it on every path
struct WindowCall {
    lvba_scans_s *sc = nullptr;
    const double *poses = nullptr;
    lvba_window_opts o{};
    const lvba_loss *loss = nullptr;  // robust loss of every window problem (lvba_lidar_ba_robust), NULL: none
    int n = 0, w = 1, n_win = 0, n_thr = 1;
    hipStream_t s = nullptr;          // the calling thread's
    lvba::hvec<hipStream_t> wstreams; // the worker threads' (n_thr > 1); they live until the call returns: the maps work on them
    lvba::hvec<WinResult> res;
    lvba::hvec<double> rel;           // [n][12] relative poses to the anchor: identity (:338), then the merged windows' (:284-299)
    lvba_voxmap_t joint_map = nullptr; // stage 1 as ONE map of all windows; the windows' maps are views into it
    lvba::hvec<DevCloud> clouds;      // [n_win] stage 3's hipMalloc'd anchor points: [w0] those of the run starting at window w0

    int start(int wi) const { return wi * w; }
    int frames(int wi) const { return std::min(w, n - wi * w); }
    void free_maps()
    {
        for (auto &R : res) if (R.map) { lvba_voxmap_destroy(R.map); R.map = nullptr; }
        if (joint_map) { lvba_voxmap_destroy(joint_map); joint_map = nullptr; }
    }
    ~WindowCall()
    {
        free_maps();
        for (auto &c : clouds) if (c.d) (void)hipFree(c.d);
        for (hipStream_t q : wstreams) if (q) lvba::StreamCache::get().release(q);
        if (s) lvba::StreamCache::get().release(s);
    }
};

// The joint passes (stage 1 and stage 3 over all windows at once) hold keys, records, indices and sort temporaries of ALL frames
// at once (~90 bytes per point, where a per-window pass needs one window's worth): they are only tried when that fits the device's
// free memory with room to spare -- a long sequence goes window by window instead of running into hipErrorOutOfMemory first.
// LVBA_WINDOW_JOINT_MAP=0: always window by window.
bool joint_fits(const WindowCall &c)
{
    static const bool on = [] { const char *e = getenv("LVBA_WINDOW_JOINT_MAP"); return !(e && !strcmp(e, "0")); }();
    if (!on || c.n_win < 2) return false;
    size_t free_b = 0, total_b = 0;
    const int64_t P = c.sc->frame_off[(size_t)c.n] - c.sc->frame_off[0];
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    if ((double)P * 96.0 > 0.5 * (double)free_b) {
        if (timing_on("window"))
            fprintf(stderr, "[window_ba] joint pass skipped: %lld points x ~96 B against %.1f GB free -> one pass per window\n",
                    (long long)P, (double)free_b / 1e9);
        return false;
    }
    return true;
}

// the window's info and starting poses (odometry) and, given its voxel map (none with merge_only), the skip rule (:258-262)
void window_init(WindowCall &c, int wi, lvba_voxmap_t map, double map_ms)
{
    WinResult &R = c.res[(size_t)wi];
    const int start = c.start(wi), cw = c.frames(wi);
    R.info = lvba_window_info{};
    R.info.start = start; R.info.n_frames = cw; R.info.anchor = -1;
    R.x.assign(c.poses + 12 * (int64_t)start, c.poses + 12 * (int64_t)(start + cw));
    R.map = map;
    if (!map) return;
    lvba_voxmap_info_t mi;
    lvba_voxmap_info(map, &mi);
    R.info.n_voxels = mi.n_voxels; R.info.n_factors = mi.n_factors;
    R.info.map_ms = map_ms;
    if (mi.n_voxels < 3 * (int64_t)cw) { // :258-262
        R.info.skipped = 1;
        lvba_voxmap_destroy(R.map);
        R.map = nullptr;
    }
}

// ---- stage 1: the voxel map at the odometry poses (:247-257), one window
int32_t stage_map(WindowCall &c, int wi, hipStream_t ws)
{
    lvba_voxmap_t map = nullptr;
    const double tw = now_ms();
    if (!c.o.merge_only) // on the worker's stream, which outlives the map
        TRY(lvba_voxmap_build_scans_on(c.sc, c.start(wi), c.frames(wi), c.poses + 12 * (int64_t)c.start(wi), &c.o.voxel, ws, &map));
    window_init(c, wi, map, now_ms() - tw);
    return LVBA_OK;
}
// ---- stage 1 for all windows at once: a root voxel is (window, key), so one sort and one pass of every kernel of the map build
// serve every window (the per-window builds are dozens of dependent launches and a dozen host round trips EACH); a window's
// part of the joint map is bit for bit what its own build gives (tests/test_gpu_window.py).  False: build them one by one.
bool stage_map_joint(WindowCall &c)
{
    const double tw = now_ms();
    if (lvba_voxmap_build_scans_joint(c.sc, 0, c.n, c.w, c.poses, &c.o.voxel, c.s, &c.joint_map) != LVBA_OK) {
        c.joint_map = nullptr; // (too many key + window bits, a bad point, ...: the per-window builds say what it is)
        return false;
    }
    const double per = (now_ms() - tw) / c.n_win;
    for (int wi = 0; wi < c.n_win; ++wi) {
        WinResult &R = c.res[(size_t)wi];
        lvba_voxmap_t view = nullptr;
        R.rc = lvba_voxmap_window_view(c.joint_map, wi, &view);
        if (R.rc != LVBA_OK) { R.err = lvba_last_error(); continue; }
        window_init(c, wi, view, per);
    }
    return true;
}

// ---- stage 2, one window at a time: damping_iter on the window's own problem (:264)
int32_t stage_lm_single(WindowCall &c, int wi, hipStream_t)
{
    WinResult &R = c.res[(size_t)wi];
    if (!R.map || R.refined) return LVBA_OK;
    const double tw = now_ms();
    lvba_voxmap_t map = R.map;
    R.map = nullptr;
    Refined r;
    TRY(refine_map(map, R.x.data(), c.o.lm, r, 0, nullptr, c.loss));
    R.info.lm_status = r.status; R.info.n_iter = r.n_iter;
    R.info.cost_first = r.cost_first; R.info.cost_last = r.cost_last;
    R.info.setup_ms = r.setup_ms;
    R.info.solve_ms = now_ms() - tw;
    R.refined = true;
    return LVBA_OK;
}
// ---- stage 2, all windows at once.  Returns LVBA_OK with `done` = false when the windows have to go one by one.
int32_t stage_lm_batched(WindowCall &c, bool &done)
{
    done = false;
    lvba::hvec<int> live;
    for (int wi = 0; wi < c.n_win; ++wi)
        if (c.res[(size_t)wi].map) live.push_back(wi);
    if (live.size() < 2) return LVBA_OK;
    const double t0 = now_ms();
    const int G = (int)live.size();
    lvba::hvec<int32_t> pose_off((size_t)G + 1, 0);
    lvba::hvec<int64_t> vox_off((size_t)G + 1, 0), fac_off((size_t)G + 1, 0);
    for (int k = 0; k < G; ++k) {
        const WinResult &R = c.res[(size_t)live[(size_t)k]];
        pose_off[(size_t)k + 1] = pose_off[(size_t)k] + R.info.n_frames;
        vox_off[(size_t)k + 1] = vox_off[(size_t)k] + R.info.n_voxels;
        fac_off[(size_t)k + 1] = fac_off[(size_t)k] + R.info.n_factors;
    }
    const int64_t V = vox_off[(size_t)G], F = fac_off[(size_t)G];
    if (F >= ((int64_t)1 << 31)) return LVBA_OK; // too large for one handle: one by one
    lvba::hvec<int64_t> off((size_t)V + 1, 0);
    lvba::hvec<int32_t> idx((size_t)F);
    lvba::hvec<double> x(12 * (size_t)pose_off[(size_t)G]);
    DevArr<double> d_clu(c.s);
    HIPCHK(d_clu.alloc(10 * (size_t)F));
    lvba::hvec<int64_t> joff; // with a joint map: its whole CSR structure in ONE pair of copies instead of two per window
    lvba::hvec<int32_t> jidx;
    if (c.joint_map) {
        lvba_voxmap_info_t ji;
        lvba_voxmap_info(c.joint_map, &ji);
        joff.resize((size_t)ji.n_voxels + 1); jidx.resize((size_t)std::max<int64_t>(ji.n_factors, 1));
        TRY(lvba_voxmap_export(c.joint_map, joff.data(), jidx.data(), nullptr, nullptr));
    }
    for (int k = 0; k < G; ++k) {
        const WinResult &R = c.res[(size_t)live[(size_t)k]];
        const int64_t v0 = vox_off[(size_t)k], f0 = fac_off[(size_t)k], nv = R.info.n_voxels, nf = R.info.n_factors;
        lvba::hvec<int64_t> o1((size_t)nv + 1);
        if (c.joint_map) {
            int64_t jv0, jv1, jf0, jf1;
            TRY(lvba_voxmap_window_range(c.joint_map, live[(size_t)k], &jv0, &jv1, &jf0, &jf1));
            memcpy(o1.data(), joff.data() + jv0, 8 * ((size_t)nv + 1));
            memcpy(idx.data() + f0, jidx.data() + jf0, 4 * (size_t)nf);
        } else
            TRY(lvba_voxmap_export(R.map, o1.data(), idx.data() + f0, nullptr, nullptr)); // CSR structure to the host, clusters stay in HBM
        for (int64_t a = 0; a <= nv; ++a) off[(size_t)(v0 + a)] = f0 + (o1[(size_t)a] - o1[0]);
        for (int64_t f = f0; f < f0 + nf; ++f) idx[(size_t)f] += pose_off[(size_t)k];
        HIPCHK(hipMemcpyAsync(d_clu + 10 * f0, lvba_voxmap_clusters(R.map), d_clu.bytes(10 * (size_t)nf), hipMemcpyDeviceToDevice, c.s));
        memcpy(x.data() + 12 * (size_t)pose_off[(size_t)k], R.x.data(), 96 * (size_t)R.info.n_frames);
    }
    HIPCHK(hipStreamSynchronize(c.s));
    const bool tm = timing_on("window");
    double tk = now_ms();
    auto mk = [&](const char *what) { if (tm) { const double t = now_ms(); fprintf(stderr, "[window_ba LM] %-16s %.3f ms\n", what, t - tk); tk = t; } };
    if (tm) fprintf(stderr, "[window_ba LM] %-16s %.3f ms\n", "export + concat", tk - t0);
    lvba_balm_t b = nullptr;
    TRY(balm_create_dev_trusted(pose_off[(size_t)G], V, off.data(), idx.data(), d_clu, c.sc->device, &b));
    struct Guard { lvba_balm_t b; ~Guard() { if (b) lvba_balm_destroy(b); } } guard{b};
    mk("create");
    TRY(lvba_balm_set_groups(b, G, pose_off.data(), vox_off.data()));
    if (c.loss) TRY(lvba_balm_set_loss(b, c.loss));
    mk("set_groups");
    lvba_balm_info_t bi;
    TRY(lvba_balm_info(b, &bi)); // the one-off set-up, timed apart
    mk("set-up");
    const double t1 = now_ms();
    lvba::hvec<int32_t> n_iter((size_t)G), status((size_t)G);
    lvba::hvec<double> first((size_t)G), last((size_t)G);
    const int32_t rc = lvba_balm_refine_groups(b, x.data(), &c.o.lm, n_iter.data(), status.data(), first.data(), last.data());
    if (rc == LVBA_NUM_FACTORIZATION) return LVBA_OK; // the windows are not independent in a broken factorisation: one by one
    if (rc < 0) return rc;
    const double t2 = now_ms();
    mk("refine_groups");
    for (int k = 0; k < G; ++k) {
        WinResult &R = c.res[(size_t)live[(size_t)k]];
        memcpy(R.x.data(), x.data() + 12 * (size_t)pose_off[(size_t)k], 96 * (size_t)R.info.n_frames);
        R.info.n_iter = n_iter[(size_t)k]; R.info.lm_status = status[(size_t)k];
        R.info.cost_first = first[(size_t)k]; R.info.cost_last = last[(size_t)k];
        R.info.setup_ms = (t1 - t0) / G; R.info.solve_ms = (t2 - t0) / G; // the joint problem's times, shared out evenly
        R.refined = true;
        lvba_voxmap_destroy(R.map);
        R.map = nullptr;
    }
    mk("results, maps freed");
    lvba_balm_destroy(guard.b);
    guard.b = nullptr;
    mk("handle destroyed");
    done = true;
    return LVBA_OK;
}

// ---- stage 3: alignment to the odometry pose of the window's first frame (:268-279) and relative poses (:284-299) into c.rel
void align_window(WindowCall &c, int wi)
{
    const int start = c.start(wi), cw = c.frames(wi);
    const double *x_odom = c.poses + 12 * (int64_t)start;
    const lvba::hvec<double> &x = c.res[(size_t)wi].x;
    const double *Ro0 = x_odom, *po0 = x_odom + 9;
    double R_align[9], p_align[3] = {0, 0, 0};
    if (c.o.use_rel) {
        mat3_mulT(Ro0, x.data(), R_align);
        for (int r = 0; r < 3; ++r)
            p_align[r] = po0[r] - (R_align[3 * r] * x[9] + R_align[3 * r + 1] * x[10] + R_align[3 * r + 2] * x[11]);
    }
    for (int j = 0; j < cw; ++j) {
        double Ra[9], pa[3];
        if (c.o.use_rel) {
            const double *Rj = x.data() + 12 * j, *pj = Rj + 9;
            mat3_mul(R_align, Rj, Ra);
            for (int r = 0; r < 3; ++r)
                pa[r] = R_align[3 * r] * pj[0] + R_align[3 * r + 1] * pj[1] + R_align[3 * r + 2] * pj[2] + p_align[r];
        } else {
            memcpy(Ra, x_odom + 12 * j, 72);
            memcpy(pa, x_odom + 12 * j + 9, 24);
        }
        double *rj = c.rel.data() + 12 * (size_t)(start + j);
        mat3T_mul(Ro0, Ra, rj);
        const double d[3] = {pa[0] - po0[0], pa[1] - po0[1], pa[2] - po0[2]};
        for (int r = 0; r < 3; ++r) rj[9 + r] = Ro0[r] * d[0] + Ro0[3 + r] * d[1] + Ro0[6 + r] * d[2];
    }
}
// Merge + down_sampling_voxel2 (tools.hpp:300-359) of the run of windows [w0, w1) in one pass: the points of every frame moved by
// its relative pose in one launch, ONE stable sort by (window, leaf key), one pick / scan / compaction into the anchor points.  A
// window's cloud is bit for bit what a run of that window alone gives: the same fp32 points, the same leaf keys, the same order
// inside a leaf (the sort is stable and a window's points keep their order), the leaves in key order.  The points of skipped
// windows (relative poses: identity) sort behind all others and are dropped.  anchor_leaf < 0.001 (tools.hpp:303): the merged
// points as they are.  *out: the clouds of the run's merged windows back to back (hipMalloc'd, as a scan set's d_pts; left empty
// when they hold no point); count[wi - w0]: window wi's points (0 when skipped).
int32_t merge_run(const WindowCall &c, int w0, int w1, hipStream_t s, DevCloud *out, int64_t *count)
{
    const lvba_scans_s *sc = c.sc;
    const int nw = w1 - w0, f0 = c.start(w0), nf = c.start(w1 - 1) + c.frames(w1 - 1) - f0;
    const int64_t p_begin = sc->frame_off[(size_t)f0], P = sc->frame_off[(size_t)(f0 + nf)] - p_begin;
    // code[window]: its rank among the run's merged windows; the skipped ones' get the code above all of those.  at: the merged
    // windows' bounds in the sorted sequence (their raw point counts: known on the host)
    lvba::hvec<uint32_t> code((size_t)nw);
    lvba::hvec<int64_t> at(1, 0);
    int G = 0;
    for (int wi = w0; wi < w1; ++wi) G += !c.res[(size_t)wi].info.skipped;
    for (int wi = w0; wi < w1; ++wi) {
        const bool skip = c.res[(size_t)wi].info.skipped;
        const int64_t np = sc->frame_off[(size_t)(c.start(wi) + c.frames(wi))] - sc->frame_off[(size_t)c.start(wi)];
        code[(size_t)(wi - w0)] = skip ? (uint32_t)G : (uint32_t)(at.size() - 1);
        count[wi - w0] = skip ? 0 : np;
        if (!skip) at.push_back(at.back() + np);
    }
    const int64_t P_live = at.back();
    if (P_live == 0) return LVBA_OK;
    const bool down = c.o.anchor_leaf >= 0.001;
    if (down && P >= ((int64_t)1 << 32)) return lvba_fail(LVBA_ERR_UNSUPPORTED, "windows [%d,%d): %lld points for 32-bit sort indices", w0, w1, (long long)P);
    const bool tm = nw > 1 && timing_on("window"); // (the per-window runs go on several host threads at once: not timed apart)
    double tj = now_ms();
    auto mark = [&](const char *what) { // (waits for the stream at every mark)
        if (!tm) return;
        (void)hipStreamSynchronize(s);
        const double t = now_ms();
        fprintf(stderr, "[window_ba merge] %-18s %.3f ms\n", what, t - tj);
        tj = t;
    };
    DevArr<double> d_rel(s); DevArr<uint32_t> d_code(s); DevArr<int64_t> d_at(s); DevArr<uint32_t> d_cnt(s);
    DevArr<float> merged(s); DevArr<int> d_err(s); DevArr<uint64_t> key(s); DevArr<double> d2(s); DevArr<uint32_t> idx(s);
    DevArr<int> d_part(s);
    DevArr<uint64_t> key_s(s); DevArr<uint32_t> order(s), flag(s), excl(s), pick(s);
    const int64_t n_slots = key_range_slots(P, 256);
    HIPCHK(d_rel.alloc(12 * (size_t)nf)); HIPCHK(merged.alloc(3 * (size_t)P));
    HIPCHK(d_rel.upload(c.rel.data() + 12 * (size_t)f0, 12 * (size_t)nf)); // (pageable sources: synchronous copies)
    if (down) {
        HIPCHK(d_code.alloc((size_t)nw)); HIPCHK(d_at.alloc((size_t)G + 1)); HIPCHK(d_cnt.alloc((size_t)G + 1));
        HIPCHK(d_err.alloc(7)); HIPCHK(key.alloc((size_t)P)); HIPCHK(d2.alloc((size_t)P)); HIPCHK(idx.alloc((size_t)P));
        HIPCHK(d_part.alloc(6 * (size_t)n_slots)); HIPCHK(d_code.upload(code.data(), (size_t)nw));
        HIPCHK(d_at.upload(at.data(), (size_t)G + 1)); HIPCHK(d_err.zero_async(7));
    }
    mark("alloc + tables");
    wba_merge_kernel<<<grid_for(P, 256), 256, 0, s>>>(P, sc->d_pts + 3 * p_begin, sc->d_frame_off + f0, nf, d_rel, c.o.anchor_leaf,
                                                      merged, down ? key : nullptr, d2, idx, d_err, d_part);
    HIPCHK(hipGetLastError());
    int64_t n_all = P_live;
    if (down) {
        key_range_reduce_kernel<<<key_range_reduce_grid(n_slots), 256, 0, s>>>(n_slots, d_part, d_err + 1);
        HIPCHK(hipGetLastError());
        int h_err[7] = {0}; // [0] error flag, [1..6] range of the biased key components
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(d_err.download(h_err, 7));
        if (h_err[0]) // (a run of several windows is retried one window at a time, so that the message names the window)
            return lvba_fail(LVBA_ERR_ARG, "window %d: a merged point is non-finite or outside +-2^20 anchor leaves", w0);
        mark("merge + range");
        // the sort runs on the bits of the leaf key that vary (voxel_internal.h) below the window's code; run leaders only
        // compare sorted keys for equality, so the re-packed ones serve as they are
        const KeyPack kp = key_pack_of(h_err + 1);
        const int cbits = G < nw ? 32 - __builtin_clz((unsigned)G) : (G > 1 ? 32 - __builtin_clz((unsigned)(G - 1)) : 0);
        const unsigned bits = (unsigned)(kp.total + cbits);
        if (bits > 64) return lvba_fail(LVBA_ERR_UNSUPPORTED, "windows [%d,%d): %u key + window bits", w0, w1, bits);
        HIPCHK(key_s.alloc((size_t)P)); HIPCHK(order.alloc((size_t)P)); HIPCHK(flag.alloc((size_t)P_live + 1));
        HIPCHK(excl.alloc((size_t)P_live + 1)); HIPCHK(pick.alloc((size_t)P_live));
        if (bits <= 32) {
            DevArr<uint32_t> k32(s);
            HIPCHK(k32.alloc((size_t)P));
            wba_compress_win_kernel<uint32_t><<<grid_for(P, 256), 256, 0, s>>>(P, key, sc->d_frame_off + f0, nf, c.w, d_code, kp,
                                                                               k32);
            HIPCHK(hipGetLastError());
            // key_s.as<uint32_t>(): the sorted 32-bit keys lie in the front half of the 64-bit buffer
            TRY(sort_pairs<uint32_t>(s, k32, key_s.as<uint32_t>(), idx, order, (size_t)P, bits));
            wba_pick_kernel<uint32_t><<<grid_for(P_live, 256), 256, 0, s>>>(P_live, key_s.as<uint32_t>(), order, d2, flag, pick);
        } else {
            wba_compress_win_kernel<uint64_t><<<grid_for(P, 256), 256, 0, s>>>(P, key, sc->d_frame_off + f0, nf, c.w, d_code, kp,
                                                                               key);
            HIPCHK(hipGetLastError());
            TRY(sort_pairs<uint64_t>(s, key, key_s, idx, order, (size_t)P, bits));
            wba_pick_kernel<uint64_t><<<grid_for(P_live, 256), 256, 0, s>>>(P_live, key_s, order, d2, flag, pick);
        }
        HIPCHK(hipGetLastError());
        mark("sort + pick");
        HIPCHK(flag.zero_async(1, P_live)); TRY(scan_excl<uint32_t>(s, flag, excl, (size_t)P_live + 1));
        wba_bounds_kernel<<<grid_for(G + 1, 256), 256, 0, s>>>(G + 1, d_at, excl, d_cnt);
        HIPCHK(hipGetLastError());
        lvba::hvec<uint32_t> cnt((size_t)G + 1);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(d_cnt.download(cnt.data(), (size_t)G + 1));
        mark("scan + counts");
        n_all = cnt[(size_t)G];
        for (int wi = w0, g = 0; wi < w1; ++wi)
            if (!c.res[(size_t)wi].info.skipped) { count[wi - w0] = (int64_t)cnt[(size_t)g + 1] - (int64_t)cnt[(size_t)g]; ++g; }
    }
    float *pts = nullptr;
    HIPCHK(hipMalloc((void **)&pts, 12 * (size_t)n_all));
    mark("hipMalloc (cloud)");
    hipError_t e = hipSuccess;
    if (down) {
        wba_compact_kernel<<<grid_for(P_live, 256), 256, 0, s>>>(P_live, flag, excl, pick, merged, pts);
        e = hipGetLastError();
    } else
        for (int wi = w0, g = 0; wi < w1 && e == hipSuccess; ++wi)
            if (!c.res[(size_t)wi].info.skipped) {
                const int64_t src = sc->frame_off[(size_t)c.start(wi)] - p_begin;
                e = hipMemcpyAsync(pts + 3 * at[(size_t)g], merged + 3 * src, merged.bytes(3 * (size_t)count[wi - w0]), hipMemcpyDeviceToDevice, s);
                ++g;
            }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(pts);
        return lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "anchor clouds: %s", hipGetErrorString(e));
    }
    mark("compact");
    *out = DevCloud{pts, n_all};
    return LVBA_OK;
}
// alignment and merge of the run of windows [w0, w1): the anchor points into c.clouds[w0], the counts into the windows' infos
int32_t stage_merge(WindowCall &c, int w0, int w1, hipStream_t s)
{
    const double tw = now_ms();
    int G = 0;
    for (int wi = w0; wi < w1; ++wi)
        if (!c.res[(size_t)wi].info.skipped) { align_window(c, wi); ++G; }
    if (G == 0) return LVBA_OK;
    lvba::hvec<int64_t> count((size_t)(w1 - w0));
    TRY(merge_run(c, w0, w1, s, &c.clouds[(size_t)w0], count.data()));
    const double per = (now_ms() - tw) / G;
    for (int wi = w0; wi < w1; ++wi) {
        lvba_window_info &info = c.res[(size_t)wi].info;
        if (info.skipped) continue;
        info.n_anchor_points = count[(size_t)(wi - w0)];
        info.merge_ms = per;
    }
    return LVBA_OK;
}
int32_t stage_merge_window(WindowCall &c, int wi, hipStream_t ws) { return stage_merge(c, wi, wi + 1, ws); }
// ---- stage 3 for all windows at once, as stage 1.  False: one pass per window.
bool stage_merge_joint(WindowCall &c)
{
    if (!joint_fits(c)) return false;
    const int32_t rc = stage_merge(c, 0, c.n_win, c.s);
    if (rc != LVBA_OK && timing_on("window")) fprintf(stderr, "[window_ba] joint merge not taken (rc %d): one pass per window\n", rc);
    return rc == LVBA_OK;
}

// a stage over all windows, on a small pool of host threads (LVBA_WINDOW_THREADS, default 4; 1 = in the calling thread), each
// with a stream of its own
void run_stage(WindowCall &c, int32_t (*stage)(WindowCall &, int, hipStream_t))
{
    std::atomic<int> next{0};
    lvba::hvec<char> visited((size_t)c.n_win, 0);
    auto worker = [&](hipStream_t ws) {
        for (int wi = next.fetch_add(1); wi < c.n_win; wi = next.fetch_add(1)) {
            WinResult &R = c.res[(size_t)wi];
            visited[(size_t)wi] = 1;
            if (R.rc < 0) continue;
            R.rc = stage(c, wi, ws);
            if (R.rc < 0) R.err = lvba_last_error();
        }
    };
    if (c.n_thr == 1) {
        worker(c.s);
        return;
    }
    struct Inhibit { Inhibit() { bs_graph_inhibit(+1); } ~Inhibit() { bs_graph_inhibit(-1); } } inhibit;
    lvba::hvec<std::thread> pool;
    for (int t = 0; t < c.n_thr; ++t)
        pool.emplace_back([&, t]() {
            if (!c.wstreams[(size_t)t] || hipSetDevice(c.sc->device) != hipSuccess) return;
            worker(c.wstreams[(size_t)t]);
            (void)hipStreamSynchronize(c.wstreams[(size_t)t]);
        });
    for (auto &th : pool) th.join();
    for (int wi = 0; wi < c.n_win; ++wi) // a thread that could not get a stream leaves its windows untouched
        if (!visited[(size_t)wi] && c.res[(size_t)wi].rc >= 0) {
            WinResult &R = c.res[(size_t)wi];
            R.rc = stage(c, wi, c.s);
            if (R.rc < 0) R.err = lvba_last_error();
        }
}

} // namespace

extern "C" void lvba_window_default_opts(lvba_window_opts *o)
{
    if (!o) return;
    o->window_size = 10;     // include/dataset_io.h:71
    o->use_rel = 1;          // config.yaml window_ba.use_window_ba_rel
    o->merge_only = 0;
    o->lm_mode = 0;
    o->anchor_leaf = 0.1;    // include/dataset_io.h:72
    lvba_voxel_default_opts(&o->voxel);
    o->voxel.voxel_size = 0.5; // stage1_root_voxel_size_, include/dataset_io.h:76
    lvba_balm_default_opts(&o->lm);
}

int32_t lvba::scans_build(int32_t device, int32_t n_frames, const int64_t *count, float *adopt, const DevCloud *src, int n_src,
                          lvba_scans_s **out)
{
    *out = nullptr;
    lvba_scans_s *sc = new (std::nothrow) lvba_scans_s();
    hipError_t e = hipSetDevice(device);
    if (!sc) {
        if (adopt && e == hipSuccess) (void)hipFree(adopt);
        return lvba_fail(LVBA_ERR_NOMEM, "host allocation failed");
    }
    sc->device = device;
    sc->n_frames = n_frames;
    sc->d_pts = adopt;
    sc->frame_off.assign((size_t)n_frames + 1, 0);
    for (int f = 0; f < n_frames; ++f) sc->frame_off[(size_t)f + 1] = sc->frame_off[(size_t)f] + count[f];
    const int64_t P = sc->frame_off[(size_t)n_frames];
    if (e == hipSuccess && !adopt) e = hipMalloc((void **)&sc->d_pts, P ? 12 * (size_t)P : 8);
    if (e == hipSuccess) e = hipMalloc((void **)&sc->d_frame_off, 8 * ((size_t)n_frames + 1));
    for (int64_t k = 0, at = 0; k < n_src && e == hipSuccess; at += src[k++].n)
        if (src[k].n > 0) e = hipMemcpy(sc->d_pts + 3 * at, src[k].d, 12 * (size_t)src[k].n, hipMemcpyDefault); // (across devices: UVA)
    if (e == hipSuccess) e = lvba::copy_h2d(sc->d_frame_off, sc->frame_off.data(), 8 * ((size_t)n_frames + 1));
    if (e != hipSuccess) {
        lvba_scans_destroy(sc);
        return lvba_fail(e == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "scan set: %s", hipGetErrorString(e));
    }
    *out = sc;
    return LVBA_OK;
}

extern "C" int32_t lvba_scans_info(lvba_scans_t sc, int32_t *n_frames, int64_t *frame_count)
{
    if (!sc) return lvba_fail(LVBA_ERR_ARG, "null handle");
    if (n_frames) *n_frames = sc->n_frames;
    if (frame_count)
        for (int f = 0; f < sc->n_frames; ++f) frame_count[f] = sc->frame_off[f + 1] - sc->frame_off[f];
    return LVBA_OK;
}

extern "C" int32_t lvba_scans_download(lvba_scans_t sc, int32_t frame, float *xyz)
{
    if (!sc || !xyz) return lvba_fail(LVBA_ERR_ARG, "null argument");
    if (frame < 0 || frame >= sc->n_frames) return lvba_fail(LVBA_ERR_ARG, "frame %d out of range [0,%d)", frame, sc->n_frames);
    HIPCHK(hipSetDevice(sc->device));
    const int64_t n = sc->frame_off[frame + 1] - sc->frame_off[frame];
    if (n > 0) HIPCHK(lvba::copy_d2h(xyz, sc->d_pts + 3 * sc->frame_off[frame], 12 * (size_t)n));
    return LVBA_OK;
}

// loss: the robust loss of every window problem (lvba_lidar_ba_robust), NULL: none
static int32_t window_ba_impl(lvba_scans_t sc, const double *poses, const lvba_window_opts *opts, double *window_poses,
                              double *rel_poses, int32_t *anchor_index, double *anchor_poses, int32_t *n_anchors,
                              lvba_scans_t *anchor_scans, lvba_window_info *win_info, const lvba_loss *loss)
{
    if (anchor_scans) *anchor_scans = nullptr;
    if (!sc || !poses || !rel_poses || !anchor_index || !anchor_poses || !n_anchors || !anchor_scans)
        return lvba_fail(LVBA_ERR_ARG, "null argument");
    WindowCall c;
    lvba_window_default_opts(&c.o);
    if (opts) c.o = *opts;
    if (c.o.window_size < 1) return lvba_fail(LVBA_ERR_ARG, "window_size must be >= 1");
    HIPCHK(hipSetDevice(sc->device));
    c.sc = sc; c.poses = poses; c.loss = loss;
    c.n = sc->n_frames; c.w = c.o.window_size; c.n_win = (c.n + c.w - 1) / c.w;
    hipStream_t s = nullptr;
    HIPCHK(lvba::StreamCache::get().acquire(&s));
    c.s = s;

    static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    for (int i = 0; i < c.n; ++i) { // rel_poses_to_anchor_.assign(total, IMUST()), anchor_index -1 (:338-339)
        memcpy(rel_poses + 12 * i, I12, sizeof I12);
        anchor_index[i] = -1;
    }
    if (window_poses) memcpy(window_poses, poses, 96 * (size_t)c.n);
    c.rel.assign(rel_poses, rel_poses + 12 * (size_t)c.n);
    c.res.resize((size_t)c.n_win);
    c.clouds.assign((size_t)c.n_win, DevCloud{nullptr, 0});
    c.n_thr = 4;
    if (const char *e = getenv("LVBA_WINDOW_THREADS")) c.n_thr = atoi(e);
    c.n_thr = std::max(1, std::min(c.n_thr, c.n_win));
    if (c.n_thr > 1) {
        c.wstreams.assign((size_t)c.n_thr, nullptr);
        for (auto &q : c.wstreams)
            if (lvba::StreamCache::get().acquire(&q) != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
    }

    const bool timing = timing_on("window"); // stage times of the whole call to stderr
    double tmark = now_ms();
    auto mark = [&](const char *what) {
        if (!timing) return;
        const double t = now_ms();
        fprintf(stderr, "[window_ba] %-18s %.3f ms\n", what, t - tmark);
        tmark = t;
    };
    auto any_failed = [&]() { for (auto &R : c.res) if (R.rc < 0) return true; return false; };
    if (c.o.merge_only || !joint_fits(c) || !stage_map_joint(c)) run_stage(c, stage_map);
    mark("voxel maps");
    if (!any_failed() && !c.o.merge_only) {
        bool done = false;
        if (c.o.lm_mode == 0) TRY(stage_lm_batched(c, done));
        if (!done) run_stage(c, stage_lm_single);
        mark(done ? "LM, all windows" : "LM, one by one");
    }
    if (!any_failed() && !stage_merge_joint(c)) run_stage(c, stage_merge_window);
    c.free_maps();
    mark("align + merge");
    for (auto &R : c.res)
        if (R.rc < 0) return lvba_fail(R.rc, "%s", R.err.c_str());
    lvba::hvec<int64_t> count; // assembled in window order
    for (int wi = 0; wi < c.n_win; ++wi) {
        WinResult &R = c.res[(size_t)wi];
        const int start = c.start(wi), cw = c.frames(wi);
        if (!R.info.skipped) {
            if (window_poses) memcpy(window_poses + 12 * (int64_t)start, R.x.data(), 96 * (size_t)cw);
            for (int j = 0; j < cw; ++j) anchor_index[start + j] = (int32_t)count.size();
            R.info.anchor = (int32_t)count.size();
            memcpy(anchor_poses + 12 * count.size(), poses + 12 * (int64_t)start, 96);
            count.push_back(R.info.n_anchor_points);
        }
        if (win_info) win_info[wi] = R.info;
    }
    memcpy(rel_poses, c.rel.data(), 96 * (size_t)c.n);
    // the anchor clouds as a scan set of their own; a single cloud (the joint pass's, or one window's) becomes its point array
    lvba::hvec<DevCloud> src;
    for (const DevCloud &cl : c.clouds) if (cl.d) src.push_back(cl);
    float *adopt = nullptr;
    if (src.size() == 1) {
        adopt = src[0].d;
        src.clear();
        for (DevCloud &cl : c.clouds) if (cl.d == adopt) cl.d = nullptr;
    }
    lvba_scans_s *out = nullptr;
    TRY(scans_build(sc->device, (int32_t)count.size(), count.data(), adopt, src.data(), (int)src.size(), &out));
    *n_anchors = out->n_frames;
    *anchor_scans = out;
    mark("anchor scan set");
    return LVBA_OK;
}

extern "C" int32_t lvba_window_ba(lvba_scans_t sc, const double *poses, const lvba_window_opts *opts, double *window_poses,
                                  double *rel_poses, int32_t *anchor_index, double *anchor_poses, int32_t *n_anchors,
                                  lvba_scans_t *anchor_scans, lvba_window_info *win_info)
{
    return window_ba_impl(sc, poses, opts, window_poses, rel_poses, anchor_index, anchor_poses, n_anchors, anchor_scans, win_info, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// The window stage over SEVERAL GPUs of one node.  The windows are independent problems (the reference solves them one after
// the other, src/lvba_system.cpp:232-302), so this is where the GPUs of a node all have work: device k takes a contiguous run
// of whole windows (lvba_window_split), a host thread per device runs lvba_window_ba on that device's scan set, the results are
// put together in window order and the anchor clouds are gathered on the first device (one device-to-device copy per share).
// A single LM refinement, by contrast, is bound by the serial chain of its band factorisation.
extern "C" int32_t lvba_window_split(int32_t n_frames, int32_t window_size, int32_t n_shares, int32_t *frame_begin)
{
    if (n_frames < 0 || window_size < 1 || n_shares < 1 || !frame_begin) return lvba_fail(LVBA_ERR_ARG, "bad argument");
    const int64_t n_win = ((int64_t)n_frames + window_size - 1) / window_size;
    for (int k = 0; k <= n_shares; ++k) { // the thread split of bavoxel.hpp:621-624, on windows
        const int64_t wb = n_win * k / n_shares;
        frame_begin[k] = (int32_t)std::min<int64_t>(n_frames, wb * window_size);
    }
    return LVBA_OK;
}

static int32_t window_ba_multi_impl(int32_t n_shares, const lvba_scans_t *scans, const double *poses, const lvba_window_opts *opts,
                                    double *window_poses, double *rel_poses, int32_t *anchor_index, double *anchor_poses,
                                    int32_t *n_anchors, lvba_scans_t *anchor_scans, lvba_window_info *win_info, const lvba_loss *loss)
{
    if (anchor_scans) *anchor_scans = nullptr;
    if (n_shares < 1 || !scans || !poses || !rel_poses || !anchor_index || !anchor_poses || !n_anchors || !anchor_scans)
        return lvba_fail(LVBA_ERR_ARG, "null argument");
    lvba_window_opts o;
    lvba_window_default_opts(&o);
    if (opts) o = *opts;
    if (o.window_size < 1) return lvba_fail(LVBA_ERR_ARG, "window_size must be >= 1");
    std::vector<int64_t> fb((size_t)n_shares + 1, 0), wb((size_t)n_shares + 1, 0);
    for (int k = 0; k < n_shares; ++k) {
        if (!scans[k]) return lvba_fail(LVBA_ERR_ARG, "share %d: null scan set", k);
        if (k + 1 < n_shares && scans[k]->n_frames % o.window_size)
            return lvba_fail(LVBA_ERR_ARG, "share %d holds %d frames: every share but the last must hold whole windows of %d (lvba_window_split)",
                             k, scans[k]->n_frames, o.window_size);
        fb[(size_t)k + 1] = fb[(size_t)k] + scans[k]->n_frames;
        wb[(size_t)k + 1] = wb[(size_t)k] + (scans[k]->n_frames + o.window_size - 1) / o.window_size;
    }
    struct Share { int32_t rc = LVBA_OK, na = 0; std::string err; lvba_scans_t anchors = nullptr; std::vector<double> ap; };
    std::vector<Share> sh((size_t)n_shares);
    // several host threads drive the device(s) from here on: no solve graph is captured meanwhile (with HIP 7.0 a capture in one
    // thread is invalidated by allocations and synchronous copies in another, block_system.hip)
    struct Inhibit { Inhibit() { bs_graph_inhibit(+1); } ~Inhibit() { bs_graph_inhibit(-1); } } inhibit;
    auto run = [&](int k) {
        Share &S = sh[(size_t)k];
        const int64_t nw = wb[(size_t)k + 1] - wb[(size_t)k];
        S.ap.assign(12 * (size_t)std::max<int64_t>(nw, 1), 0.0);
        S.rc = window_ba_impl(scans[k], poses + 12 * fb[(size_t)k], &o, window_poses ? window_poses + 12 * fb[(size_t)k] : nullptr,
                              rel_poses + 12 * fb[(size_t)k], anchor_index + fb[(size_t)k], S.ap.data(), &S.na, &S.anchors,
                              win_info ? win_info + wb[(size_t)k] : nullptr, loss);
        if (S.rc < 0) S.err = lvba_last_error();
    };
    {
        std::vector<std::thread> th;
        for (int k = 1; k < n_shares; ++k) th.emplace_back(run, k);
        run(0);
        for (auto &t : th) t.join();
    }
    auto drop = [&]() { for (auto &S : sh) if (S.anchors) { lvba_scans_destroy(S.anchors); S.anchors = nullptr; } };
    for (int k = 0; k < n_shares; ++k)
        if (sh[(size_t)k].rc < 0) {
            const int32_t rc = sh[(size_t)k].rc;
            const std::string msg = sh[(size_t)k].err;
            drop();
            return lvba_fail(rc, "share %d: %s", k, msg.c_str());
        }
    // window order: anchors of share k come after those of the shares before it
    int32_t base = 0;
    for (int k = 0; k < n_shares; ++k) {
        const Share &S = sh[(size_t)k];
        for (int64_t f = fb[(size_t)k]; f < fb[(size_t)k + 1]; ++f)
            if (anchor_index[f] >= 0) anchor_index[f] += base;
        if (win_info)
            for (int64_t w = wb[(size_t)k]; w < wb[(size_t)k + 1]; ++w) {
                win_info[w].start += (int32_t)fb[(size_t)k];
                if (win_info[w].anchor >= 0) win_info[w].anchor += base;
            }
        memcpy(anchor_poses + 12 * (size_t)base, S.ap.data(), 96 * (size_t)S.na);
        base += S.na;
    }
    // the anchor clouds as ONE scan set on the first share's device
    lvba::hvec<int64_t> count;
    lvba::hvec<DevCloud> src;
    for (const Share &S : sh) {
        for (int f = 0; f < S.na; ++f) count.push_back(S.anchors->frame_off[(size_t)f + 1] - S.anchors->frame_off[(size_t)f]);
        src.push_back({S.anchors->d_pts, S.anchors->frame_off[(size_t)S.na]});
    }
    lvba_scans_s *out = nullptr;
    const int32_t rc = scans_build(scans[0]->device, base, count.data(), nullptr, src.data(), n_shares, &out);
    drop();
    if (rc != LVBA_OK) return rc;
    *n_anchors = base;
    *anchor_scans = out;
    return LVBA_OK;
}

extern "C" int32_t lvba_window_ba_multi(int32_t n_shares, const lvba_scans_t *scans, const double *poses, const lvba_window_opts *opts,
                                        double *window_poses, double *rel_poses, int32_t *anchor_index, double *anchor_poses,
                                        int32_t *n_anchors, lvba_scans_t *anchor_scans, lvba_window_info *win_info)
{
    return window_ba_multi_impl(n_shares, scans, poses, opts, window_poses, rel_poses, anchor_index, anchor_poses, n_anchors, anchor_scans,
                                win_info, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// LvbaSystem::runLidarBA (src/lvba_system.cpp:312-410) without the ROS/visualisation calls: window BA -> anchors, then the
// global stages (stage 1 optional, stage 2) each re-cutting the anchor clouds at the current anchor poses with that stage's
// voxel size / eigen ratios and running damping_iter over all anchors, then every frame's pose = anchor o rel (:393-404).
extern "C" void lvba_lidar_ba_default_opts(lvba_lidar_ba_opts *o)
{
    if (!o) return;
    lvba_window_default_opts(&o->window);
    o->window_enable = 1;                                        // include/dataset_io.h:70
    o->stage1_enable = 1;                                        // include/dataset_io.h:75
    o->stage_voxel_size[0] = 0.5; o->stage_voxel_size[1] = 0.5;  // include/dataset_io.h:76,79
    const float r1[4] = {0.3f, 0.1f, 0.06f, 0.03f}, r2[4] = {0.08f, 0.08f, 0.08f, 0.08f}; // :77,:80
    for (int k = 0; k < 4; ++k) { o->stage_eigen_ratio[0][k] = r1[k]; o->stage_eigen_ratio[1][k] = r2[k]; }
    lvba_balm_default_opts(&o->lm);
}

// n_shares == 1: the whole sequence on scs[0]'s device; > 1: the window stage over the shares (lvba_window_ba_multi), the global
// stages -- single problems over all anchors -- on the first share's device, where the anchor clouds are gathered

// frame priors -> priors on the anchors of the global stages: frame f = anchor a(f) o rel_f, so T_f O = T_a (rel_f o O) exactly.
// Frames of skipped windows (anchor -1) and relative priors inside one anchor (constant at this stage) are dropped.
static void priors_to_anchors(int32_t n, const lvba_prior *fp, const int32_t *aidx, const double *rel, std::vector<lvba_prior> &out)
{
    out.clear();
    auto compose = [](const double *A, const double *B, double *C) { // C = A o B
        double O[12];
        mat3_mul(A, B, O);
        for (int q = 0; q < 3; ++q) O[9 + q] = A[3 * q] * B[9] + A[3 * q + 1] * B[10] + A[3 * q + 2] * B[11] + A[9 + q];
        memcpy(C, O, sizeof O);
    };
    for (int32_t k = 0; k < n; ++k) {
        lvba_prior q = fp[k];
        const bool relk = q.kind == LVBA_PRIOR_RELATIVE;
        const int32_t ai = aidx[q.i], aj = relk ? aidx[q.j] : ai;
        if (ai < 0 || aj < 0 || (relk && ai == aj)) continue;
        double o[12];
        lvba::prior_offset_or_identity(fp[k].offset_i, o);
        compose(rel + 12 * (size_t)q.i, o, q.offset_i);
        q.i = ai;
        if (relk) {
            lvba::prior_offset_or_identity(fp[k].offset_j, o);
            compose(rel + 12 * (size_t)fp[k].j, o, q.offset_j);
            q.j = aj;
        }
        out.push_back(q);
    }
}

static int32_t lidar_ba_impl(int32_t n_shares, const lvba_scans_t *scs, const double *poses_in, const lvba_lidar_ba_opts *opts,
                             double *poses_out, lvba_lidar_ba_report *rep, int32_t n_priors = 0, const lvba_prior *priors = nullptr,
                             lvba_prior *anchor_priors = nullptr, int32_t *n_used = nullptr, int32_t *n_dropped = nullptr,
                             const lvba_loss *window_loss = nullptr, const lvba_loss *stage_loss = nullptr)
{
    if (n_shares < 1 || !scs || !scs[0] || !poses_in || !poses_out) return lvba_fail(LVBA_ERR_ARG, "null argument");
    lvba_lidar_ba_opts o;
    lvba_lidar_ba_default_opts(&o);
    if (opts) o = *opts;
    lvba_scans_t sc = scs[0];
    int n = 0;
    for (int k = 0; k < n_shares; ++k) {
        if (!scs[k]) return lvba_fail(LVBA_ERR_ARG, "share %d: null scan set", k);
        n += scs[k]->n_frames;
    }
    if (n_shares > 1 && !o.window_enable)
        return lvba_fail(LVBA_ERR_ARG, "several shares need the window stage (window_enable = 0 cuts the RAW scans in the global stages: one device)");
    TRY(lvba::prior_validate(n_priors, priors, n));
    TRY(lvba::loss_validate(window_loss, "window_loss"));
    TRY(lvba::loss_validate(stage_loss, "stage_loss"));
    lvba_lidar_ba_report r{};
    r.n_frames = n;
    lvba::hvec<double> rel(12 * (size_t)n), anchor_poses;
    lvba::hvec<int32_t> aidx((size_t)n);
    lvba_scans_t anchors = nullptr;
    int32_t na = 0;
    double t0 = now_ms();
    if (o.window_enable) {
        const int nw = (n + o.window.window_size - 1) / std::max(1, o.window.window_size);
        anchor_poses.resize(12 * (size_t)std::max(nw, 1));
        lvba::hvec<lvba_window_info> wi((size_t)std::max(nw, 1));
        if (n_shares == 1) TRY(window_ba_impl(sc, poses_in, &o.window, nullptr, rel.data(), aidx.data(), anchor_poses.data(), &na, &anchors, wi.data(), window_loss));
        else TRY(window_ba_multi_impl(n_shares, scs, poses_in, &o.window, nullptr, rel.data(), aidx.data(), anchor_poses.data(), &na, &anchors, wi.data(), window_loss));
        r.n_windows = nw;
        for (int k = 0; k < nw; ++k) r.n_windows_skipped += wi[k].skipped;
    } else { // :221-229: every frame is its own anchor
        static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        anchor_poses.assign(poses_in, poses_in + 12 * (size_t)n);
        for (int i = 0; i < n; ++i) { memcpy(rel.data() + 12 * i, I12, sizeof I12); aidx[i] = i; }
        na = n;
    }
    r.n_anchors = na;
    r.window_ms = now_ms() - t0;
    std::vector<lvba_prior> ap;
    priors_to_anchors(n_priors, priors, aidx.data(), rel.data(), ap);
    if (n_used) *n_used = (int32_t)ap.size();
    if (n_dropped) *n_dropped = n_priors - (int32_t)ap.size();
    if (anchor_priors && !ap.empty()) memcpy(anchor_priors, ap.data(), ap.size() * sizeof(lvba_prior));
    struct AnchorGuard { lvba_scans_t a; ~AnchorGuard() { lvba_scans_destroy(a); } } guard{anchors};
    lvba_scans_t cut = o.window_enable ? anchors : sc;
    if (na > 0)
        for (int idx = o.stage1_enable ? 0 : 1; idx < 2; ++idx) {
            t0 = now_ms();
            lvba_voxel_opts vo = o.window.voxel;
            vo.voxel_size = o.stage_voxel_size[idx];
            for (int k = 0; k < 4; ++k) vo.eigen_ratio[k] = o.stage_eigen_ratio[idx][k];
            lvba_voxmap_t map = nullptr;
            TRY(lvba_voxmap_build_scans(cut, 0, na, anchor_poses.data(), &vo, &map));
            lvba_voxmap_info_t mi;
            lvba_voxmap_info(map, &mi);
            r.stage_voxels[idx] = mi.n_voxels; r.stage_factors[idx] = mi.n_factors; r.stage_ran[idx] = 1;
            if (mi.n_voxels == 0) {
                // nothing admitted at this stage's voxel size: upstream, damping_iter over an empty VOX_HESS averages 0 / 0
                // (bavoxel.hpp:634-635), every step is rejected on the NaN cost and the poses come out as they went in
                // (src/lvba_system.cpp:386) -- the stage is a no-op, the next stage and the anchor / rel composition still run
                lvba_voxmap_destroy(map);
                r.stage_ran[idx] = 0;
                r.stage_ms[idx] = now_ms() - t0;
                continue;
            }
            Refined rr;
            TRY(refine_map(map, anchor_poses.data(), o.lm, rr, (int32_t)ap.size(), ap.data(), stage_loss));
            r.stage_status[idx] = rr.status; r.stage_iters[idx] = rr.n_iter;
            r.stage_cost_first[idx] = rr.cost_first; r.stage_cost_last[idx] = rr.cost_last;
            r.stage_ms[idx] = now_ms() - t0;
        }
    memcpy(poses_out, poses_in, 96 * (size_t)n); // optimized_x_buf_ = x_buf_full (:393)
    for (int i = 0; i < n; ++i) {
        const int a = aidx[i];
        if (a < 0 || a >= na) continue;
        const double *A = anchor_poses.data() + 12 * (size_t)a, *L = rel.data() + 12 * (size_t)i;
        double *O = poses_out + 12 * (size_t)i;
        mat3_mul(A, L, O);
        for (int q = 0; q < 3; ++q) O[9 + q] = A[3 * q] * L[9] + A[3 * q + 1] * L[10] + A[3 * q + 2] * L[11] + A[9 + q];
    }
    if (rep) *rep = r;
    return LVBA_OK;
}

extern "C" int32_t lvba_lidar_ba(lvba_scans_t sc, const double *poses_in, const lvba_lidar_ba_opts *opts, double *poses_out,
                                 lvba_lidar_ba_report *rep)
{
    return lidar_ba_impl(1, &sc, poses_in, opts, poses_out, rep);
}

extern "C" int32_t lvba_lidar_ba_multi(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in,
                                       const lvba_lidar_ba_opts *opts, double *poses_out, lvba_lidar_ba_report *rep)
{
    return lidar_ba_impl(n_shares, scans, poses_in, opts, poses_out, rep);
}

extern "C" int32_t lvba_lidar_ba_priors(lvba_scans_t sc, const double *poses_in, const lvba_lidar_ba_opts *opts, int32_t n_priors,
                                        const lvba_prior *priors, double *poses_out, lvba_lidar_ba_report *rep, lvba_prior *anchor_priors,
                                        int32_t *n_used, int32_t *n_dropped)
{
    return lidar_ba_impl(1, &sc, poses_in, opts, poses_out, rep, n_priors, priors, anchor_priors, n_used, n_dropped);
}

extern "C" int32_t lvba_lidar_ba_multi_priors(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in,
                                              const lvba_lidar_ba_opts *opts, int32_t n_priors, const lvba_prior *priors, double *poses_out,
                                              lvba_lidar_ba_report *rep, lvba_prior *anchor_priors, int32_t *n_used, int32_t *n_dropped)
{
    return lidar_ba_impl(n_shares, scans, poses_in, opts, poses_out, rep, n_priors, priors, anchor_priors, n_used, n_dropped);
}

extern "C" int32_t lvba_lidar_ba_robust(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in, const lvba_lidar_ba_opts *opts,
                                        const lvba_loss *window_loss, const lvba_loss *stage_loss, int32_t n_priors, const lvba_prior *priors,
                                        double *poses_out, lvba_lidar_ba_report *rep, lvba_prior *anchor_priors, int32_t *n_used,
                                        int32_t *n_dropped)
{
    return lidar_ba_impl(n_shares, scans, poses_in, opts, poses_out, rep, n_priors, priors, anchor_priors, n_used, n_dropped, window_loss,
                         stage_loss);
}
