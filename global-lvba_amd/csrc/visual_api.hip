// visual_api.hip -- visual half of the C-ABI (include/lvba_hip.h): packing of the landmark/observation problem and
// the trust-region Levenberg-Marquardt driver that replaces ceres::Solve in LvbaSystem::optimizeCameraPoses
// (reference src/lvba_system.cpp:1571-1665).  The control flow restates Ceres 2.1.0's TrustRegionMinimizer +
// LevenbergMarquardtStrategy (not in /root/reference; restated from its published sources):
// Jacobi scaling fixed at iteration 0, LM diagonal sqrt(clamp(diag J^T J)/radius),
// parameter/function tolerance checks before the accept test, radius /= max(1/3, 1-(2 rho-1)^3) on success and
// /= 2,4,8.. on failure.  Host logic only; arithmetic runs in visual_kernels.hip, balm_pair_kernel and ldlt.hip.
// Robust losses (lvba_visual_set_loss) follow Ceres 2.1's ResidualBlock::Evaluate + Corrector, restated in visual_loss.h: a
// block contributes 1/2 rho(s) to every cost this driver compares, and (r~, J~) to everything built from the linearisation.
// Camera pose priors (lvba_visual_set_priors; visual_prior_device.h, visual_priors.hip) are further residual blocks with a
// trivial loss on one or two cameras: their rows count in the Jacobi scaling, the LM diagonal, the gradient max, the reduced
// system, the model cost change and every cost.  A handle with priors runs the sharded form of the camera kernels (per-camera
// sums first, LM diagonal and gradient max after the priors have been added to them); one without launches nothing new.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "host_arena.h"
#include "block_system.h"
#include "prior_tables.h"

using namespace lvba;
#define fail lvba_fail

struct lvba_visual_s {
    BlockSys bs;
    int32_t M = 0;
    int64_t T = 0, Ta = 0, O = 0;
    lvba::hvec<int64_t> act;      // active landmark -> caller track index
    lvba::hvec<int64_t> h_off;    // CSR of the active landmarks (host, kept until finalize)
    lvba::hvec<int32_t> h_cam;    // caller camera index per kept observation
    lvba::hvec<int64_t> obs_src;  // caller observation index (relative to obs_off[0]) per kept observation
    int64_t O_all = 0;            // caller observations, kept or not
    int32_t loss_kind[2] = {0, 0}; // [0] reprojection, [1] plane: LVBA_LOSS_*; scale 0 on TRIVIAL
    double loss_scale[2] = {0.0, 0.0};
    bool finalized = false;
    int32_t cam_form = -1;         // LVBA_VIS_CAM_FORM=0|1 as read at finalize; -1: the rule (vis_eval_layout)
    bool have_lin = false;         // bs holds the reduced system of an lvba_visual_linearize (lvba_visual_solve); a refine replaces it
    double intr[8] = {}, sig_px = 0.5, sig_pl = 0.01;
    // camera pose priors (lvba_visual_set_priors): as the caller gave them, and bound to the solver order (bind_priors)
    std::vector<lvba_prior> priors;
    PriorTables pt;                     // their records and scatter tables on the device
    VisPriorDev vp;                     // what the kernels take: tab = pt.dev
    lvba::hvec<int64_t> pat_slots;      // blocks the pair pass writes or the packed all-reduce carries (sorted; bind_priors)
    bool pat_known = false;
    double *d_pscal = nullptr;          // [2] the priors' trial cost and model cost change of one LM iteration
    // device
    int64_t *d_off = nullptr;
    int32_t *d_cam = nullptr, *d_track_of_obs = nullptr;
    double *d_uv = nullptr, *d_plane = nullptr, *d_uv_cm = nullptr;
    double *d_Jc = nullptr, *d_Jp = nullptr, *d_r = nullptr, *d_rpl = nullptr, *d_Jpl = nullptr;
    double *d_sc_cam = nullptr, *d_sc_pt = nullptr, *d_Lp = nullptr, *d_zp = nullptr, *d_step_p = nullptr, *d_part = nullptr;
    double *d_q = nullptr, *d_t = nullptr, *d_X = nullptr, *d_q2 = nullptr, *d_t2 = nullptr, *d_X2 = nullptr;
    double *d_blkpart = nullptr;   // per-workgroup partials of the scalar reductions
    double *d_scal = nullptr;      // [0]=cost(x) [1]=cost(cand) [2]=model change [3]=|step|^2 [4]=|x|^2
    unsigned long long *d_gmax = nullptr;
    double *d_camsum = nullptr, *d_colsum = nullptr; // sharded runs: per-camera sums awaiting the other ranks' tracks
    double *d_out = nullptr;       // export staging
    double *h_pin = nullptr;
    double *hq = nullptr, *ht = nullptr, *hX = nullptr; // host staging in solver order: ONE pinned block (h_stage), so the state
    double *h_stage = nullptr;                          // uploads / downloads are DMA transfers, not pageable copies

    VisDev dev() const
    {
        VisDev d;
        d.M = M; d.S = bs.S; d.band_blocks = bs.Bb; d.fixed_cam = bs.iperm.empty() ? 0 : bs.iperm[0];
        d.Ta = Ta; d.O = O; d.off = d_off; d.cam = d_cam; d.track_of_obs = d_track_of_obs; d.uv = d_uv; d.uv_cm = d_uv_cm; d.plane = d_plane;
        for (int e = 0; e < 8; ++e) d.intr[e] = intr[e];
        d.inv_sig_px = 1.0 / sig_px; d.inv_sig_pl = 1.0 / std::max(1e-9, sig_pl); // utils.hpp:131
        d.Jc = d_Jc; d.Jp = d_Jp; d.r = d_r; d.rpl = d_rpl; d.Jpl = d_Jpl; d.sc_cam = d_sc_cam; d.sc_pt = d_sc_pt;
        d.Lp = d_Lp; d.zp = d_zp; d.step_p = d_step_p;
        d.csc_off = bs.d_csc_off; d.csc_f = bs.d_csc_f; d.group_of_pos = bs.d_group_of_pos; d.pos_of = bs.d_pos_of;
        d.Y = bs.d_Y; d.part = d_part;
        d.dist = (bs.distributed() || vp.tab.n > 0) ? 1 : 0; d.count_cams = bs.rank == 0 ? 1 : 0; d.camsum = d_camsum; d.colsum = d_colsum;
        d.robust = (loss_kind[0] != LVBA_LOSS_TRIVIAL || loss_kind[1] != LVBA_LOSS_TRIVIAL) ? 1 : 0;
        for (int f = 0; f < 2; ++f) { d.loss_kind[f] = loss_kind[f]; d.loss_scale[f] = loss_scale[f]; }
        d.cam_form = cam_form;
        return d;
    }
};

extern "C" void lvba_visual_default_opts(lvba_visual_opts *o)
{
    if (!o) return;
    o->max_iter = 50; o->reserved = 0; o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
}

extern "C" int32_t lvba_visual_destroy(lvba_visual_t h)
{
    if (!h) return LVBA_OK;
    hipSetDevice(h->bs.device);
    if (h->bs.stream) hipStreamSynchronize(h->bs.stream);
    void *ptrs[] = {h->d_off, h->d_cam, h->d_track_of_obs, h->d_uv, h->d_uv_cm, h->d_plane, h->d_Jc, h->d_Jp, h->d_r, h->d_rpl, h->d_Jpl,
                    h->d_sc_cam, h->d_sc_pt, h->d_Lp, h->d_zp, h->d_step_p, h->d_part, h->d_q, h->d_t, h->d_X, h->d_q2,
                    h->d_t2, h->d_X2, h->d_blkpart, h->d_scal, h->d_gmax, h->d_out, h->d_camsum, h->d_colsum, h->d_pscal};
    for (void *p : ptrs)
        if (p) lvba::DevicePool::get().free(p);
    h->pt.free_mem();
    if (h->h_pin) hipHostFree(h->h_pin);
    if (h->h_stage) hipHostFree(h->h_stage);
    bs_destroy(h->bs);
    delete h;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_create(int32_t n_cams, int64_t n_tracks, const int64_t *obs_off, const int32_t *obs_cam,
                                      const double *obs_uv, const double *plane, const uint8_t *valid, const double intr[8],
                                      double sigma_px, double sigma_plane, int32_t device, lvba_visual_t *out)
{
    if (!out) return fail(LVBA_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n_cams < 1 || n_tracks < 0 || !obs_off || !plane || !valid || !intr) return fail(LVBA_ERR_ARG, "bad sizes or NULL arrays");
    if (!(sigma_px > 0.0)) return fail(LVBA_ERR_ARG, "sigma_px must be > 0");
    const int64_t base = obs_off[0];
    const int64_t Oall = obs_off[n_tracks] - base;
    if (Oall > 0 && (!obs_cam || !obs_uv)) return fail(LVBA_ERR_ARG, "observation arrays are NULL");
    TRY(lvba::check_device(device));
    lvba_visual_s *h = new (std::nothrow) lvba_visual_s();
    if (!h) return fail(LVBA_ERR_NOMEM, "host allocation failed");
    h->M = n_cams; h->T = n_tracks; h->sig_px = sigma_px; h->sig_pl = sigma_plane;
    memcpy(h->intr, intr, 8 * sizeof(double));
    // keep only landmarks with a valid plane, together with their observations (src/lvba_system.cpp:1598-1603)
    lvba::hvec<double> uv, pl;
    h->h_off.push_back(0);
    for (int64_t i = 0; i < n_tracks; ++i) {
        if (obs_off[i + 1] < obs_off[i]) { delete h; return fail(LVBA_ERR_ARG, "obs_off is not monotone at %lld", (long long)i); }
        if (!valid[i]) continue;
        for (int64_t o = obs_off[i] - base; o < obs_off[i + 1] - base; ++o) {
            if (obs_cam[o] < 0 || obs_cam[o] >= n_cams) { delete h; return fail(LVBA_ERR_ARG, "obs_cam[%lld] = %d out of range", (long long)o, obs_cam[o]); }
            h->h_cam.push_back(obs_cam[o]);
            h->obs_src.push_back(o);
            uv.push_back(obs_uv[2 * o]);
            uv.push_back(obs_uv[2 * o + 1]);
        }
        h->act.push_back(i);
        h->h_off.push_back((int64_t)h->h_cam.size());
        for (int e = 0; e < 4; ++e) pl.push_back(plane[4 * i + e]);
    }
    h->Ta = (int64_t)h->act.size();
    h->O = (int64_t)h->h_cam.size();
    h->O_all = Oall;
    auto bail = [&](int32_t rc) { lvba_visual_destroy(h); return rc; };
#define CTRY(expr) do { int32_t rc_ = (expr); if (rc_ != LVBA_OK) return bail(rc_); } while (0)
#define CHIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(e_ == hipErrorOutOfMemory ? LVBA_ERR_NOMEM : LVBA_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    CTRY(bs_init(h->bs, device));
    BlockSys &bs = h->bs;
    const int64_t Ta = h->Ta, O = h->O, M = n_cams;
    CTRY(bs_dmalloc(bs, &h->d_off, Ta + 1));
    CTRY(bs_dmalloc(bs, &h->d_cam, O));
    CTRY(bs_dmalloc(bs, &h->d_track_of_obs, O));
    CTRY(bs_dmalloc(bs, &h->d_uv, 2 * O));
    CTRY(bs_dmalloc(bs, &h->d_plane, 4 * Ta));
    CHIP(hipMemcpy(h->d_off, h->h_off.data(), (size_t)(Ta + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (O) CHIP(hipMemcpy(h->d_uv, uv.data(), (size_t)(2 * O) * sizeof(double), hipMemcpyHostToDevice));
    if (Ta) CHIP(hipMemcpy(h->d_plane, pl.data(), (size_t)(4 * Ta) * sizeof(double), hipMemcpyHostToDevice));
    {
        lvba::hvec<int32_t> too((size_t)O);
        for (int64_t i = 0; i < Ta; ++i)
            for (int64_t o = h->h_off[i]; o < h->h_off[i + 1]; ++o) too[o] = (int32_t)i;
        if (O) CHIP(hipMemcpy(h->d_track_of_obs, too.data(), (size_t)O * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    CTRY(bs_dmalloc(bs, &h->d_Jc, 12 * O)); CTRY(bs_dmalloc(bs, &h->d_Jp, 6 * O)); CTRY(bs_dmalloc(bs, &h->d_r, 2 * O));
    CTRY(bs_dmalloc(bs, &h->d_rpl, Ta)); CTRY(bs_dmalloc(bs, &h->d_Jpl, 3 * Ta));
    CTRY(bs_dmalloc(bs, &h->d_sc_cam, 6 * M)); CTRY(bs_dmalloc(bs, &h->d_sc_pt, 3 * Ta));
    CTRY(bs_dmalloc(bs, &h->d_Lp, 6 * Ta)); CTRY(bs_dmalloc(bs, &h->d_zp, 3 * Ta)); CTRY(bs_dmalloc(bs, &h->d_step_p, 3 * Ta));
    CTRY(bs_dmalloc(bs, &h->d_q, 4 * M)); CTRY(bs_dmalloc(bs, &h->d_t, 3 * M)); CTRY(bs_dmalloc(bs, &h->d_X, 3 * Ta));
    CTRY(bs_dmalloc(bs, &h->d_q2, 4 * M)); CTRY(bs_dmalloc(bs, &h->d_t2, 3 * M)); CTRY(bs_dmalloc(bs, &h->d_X2, 3 * Ta));
    CTRY(bs_dmalloc(bs, &h->d_blkpart, 2 * ((O + 4 * Ta + M) / 256 + 4))); // vis_back_kernel: four lanes per landmark
    CTRY(bs_dmalloc(bs, &h->d_scal, 16));
    CTRY(bs_dmalloc(bs, &h->d_gmax, 2));
    CTRY(bs_dmalloc(bs, &h->d_out, 36 * (int64_t)M + 16));
    CTRY(bs_dmalloc(bs, &h->d_camsum, 12 * (int64_t)M));
    CTRY(bs_dmalloc(bs, &h->d_colsum, 6 * (int64_t)M));
    CTRY(bs_dmalloc(bs, &h->d_pscal, 2));
    CHIP(hipHostMalloc((void **)&h->h_pin, 16 * sizeof(double), hipHostMallocDefault));
#undef CTRY
#undef CHIP
    *out = h;
    return LVBA_OK;
}

static int32_t bind_priors(lvba_visual_s *h);

static int32_t finalize(lvba_visual_s *h)
{
    if (h->finalized) return LVBA_OK;
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    // read once, here: a launch never looks at the environment; a refused value leaves the handle as it was
    int32_t form_env = -1;
    TRY(env_int_in_range("LVBA_VIS_CAM_FORM", 0, 1, &form_env));
    bs.spd = true; // S = sum Jc^T Jc + D^2 - sum Y Y^T is the Schur complement of a positive definite matrix
    TRY(bs_build(bs, h->M, h->Ta, h->h_off.data(), h->h_cam.data()));
    h->cam_form = form_env;
    {
        lvba::hvec<int32_t> cam((size_t)h->O);
        for (int64_t o = 0; o < h->O; ++o) cam[o] = bs.iperm[h->h_cam[o]];
        if (h->O) HIPCHK(hipMemcpy(h->d_cam, cam.data(), (size_t)h->O * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    TRY(bs_dmalloc(bs, &h->d_part, (int64_t)h->M * bs.S * 40));
    TRY(bs_dmalloc(bs, &h->d_uv_cm, 2 * std::max<int64_t>(1, h->O)));
    vis_launch_gather_uv(h->dev(), h->d_uv_cm, bs.stream);
    lvba::hvec<int32_t>().swap(h->h_cam);
    h->finalized = true;
    if (!h->priors.empty()) TRY(bind_priors(h));
    return LVBA_OK;
}

// caller arrays -> device state in solver order
static int32_t import_state(lvba_visual_s *h, const double *q, const double *t, const double *X)
{
    BlockSys &bs = h->bs;
    if (!h->h_stage) {
        HIPCHK(hipHostMalloc((void **)&h->h_stage, (7 * (size_t)h->M + 3 * (size_t)h->Ta + 8) * sizeof(double), hipHostMallocDefault));
        h->hq = h->h_stage; h->ht = h->hq + 4 * (size_t)h->M; h->hX = h->ht + 3 * (size_t)h->M;
    }
    for (int c = 0; c < h->M; ++c) {
        const int I = bs.iperm[c];
        for (int e = 0; e < 4; ++e) h->hq[4 * I + e] = q[4 * c + e];
        for (int e = 0; e < 3; ++e) h->ht[3 * I + e] = t[3 * c + e];
    }
    for (int64_t i = 0; i < h->Ta; ++i)
        for (int e = 0; e < 3; ++e) h->hX[3 * i + e] = X[3 * h->act[i] + e];
    HIPCHK(hipMemcpyAsync(h->d_q, h->hq, 4 * (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, bs.stream));
    HIPCHK(hipMemcpyAsync(h->d_t, h->ht, 3 * (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, bs.stream));
    if (h->Ta) HIPCHK(hipMemcpyAsync(h->d_X, h->hX, 3 * (size_t)h->Ta * sizeof(double), hipMemcpyHostToDevice, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream)); // the host staging vectors may be reused
    return LVBA_OK;
}

static int32_t export_state(lvba_visual_s *h, double *q, double *t, double *X)
{
    BlockSys &bs = h->bs;
    HIPCHK(hipMemcpyAsync(h->hq, h->d_q, 4 * (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipMemcpyAsync(h->ht, h->d_t, 3 * (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    if (h->Ta) HIPCHK(hipMemcpyAsync(h->hX, h->d_X, 3 * (size_t)h->Ta * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    for (int c = 0; c < h->M; ++c) {
        const int I = bs.iperm[c];
        const double *s = &h->hq[4 * I];
        const double nq = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3]); // q_eig.normalize(), :1653
        for (int e = 0; e < 4; ++e) q[4 * c + e] = s[e] / nq;
        for (int e = 0; e < 3; ++e) t[3 * c + e] = h->ht[3 * I + e];
    }
    for (int64_t i = 0; i < h->Ta; ++i)
        for (int e = 0; e < 3; ++e) X[3 * h->act[i] + e] = h->hX[3 * i + e];
    return LVBA_OK;
}

// ---- the steps of a linearisation / an iteration that need the other ranks' track shards (no-ops on one rank) -------------
static int32_t enqueue_colnorms(lvba_visual_s *h)
{
    BlockSys &bs = h->bs;
    const VisDev d = h->dev();
    if (!d.dist) { vis_launch_colnorms(d, bs.stream); return LVBA_OK; }
    vis_launch_colsums(d, bs.stream);
    vprior_launch_colsum_add(h->vp, h->d_colsum, bs.stream); // the prior rows' columns (vprior_launch_lin0 has run)
    TRY(bs_allreduce(bs, h->d_colsum, 6 * (size_t)h->M));
    vis_launch_colnorm_finish(d, bs.stream);
    return LVBA_OK;
}
static int32_t enqueue_reduced_system(lvba_visual_s *h, double radius, const lvba_visual_opts &o)
{
    BlockSys &bs = h->bs;
    const VisDev d = h->dev();
    vis_launch_reduced_system(d, bs.pair_dev(), h->d_q, h->d_t, h->d_X, radius, o.min_lm_diagonal, o.max_lm_diagonal, bs.Hblk(), bs.hblk_doubles, bs.g(),
                              h->d_gmax, bs.distributed(), bs.stream);
    if (!d.dist) return LVBA_OK;
    // camera priors: after the Schur elimination, into the blocks of S, the reduced rhs and the per-camera sums (one rank adds them)
    vprior_launch_eval(h->vp, h->d_q, h->d_t, h->d_sc_cam, h->M, bs.Hblk(), bs.g(), h->d_camsum, bs.stream);
    TRY(bs_allreduce_hg(bs));                                   // [S blocks | reduced rhs]: sums over the track shards
    TRY(bs_allreduce(bs, h->d_camsum, 12 * (size_t)h->M));      // diag(Jc^T Jc), Jc^T r
    vis_launch_cam_finish(d, radius, o.min_lm_diagonal, o.max_lm_diagonal, bs.Hblk(), h->d_q, h->d_gmax, bs.stream);
    if (bs.distributed()) TRY(bs_comm_allreduce(bs, h->d_gmax, 1, ncclInt64, ncclMax)); // bit patterns of non-negative doubles order like integers
    return LVBA_OK;
}
static int32_t allreduce_scalars(lvba_visual_s *h, int first, int count)
{
    if (!h->bs.distributed()) return LVBA_OK;
    return bs_allreduce(h->bs, h->d_scal + first, (size_t)count);
}

// Sharded handles: every rank must use the same losses and the same camera priors: one MAX all-reduce (bs_ranks_agree) of the
// kinds, the scale bits, the priors' count and the hash of their records (reserved fields are stored as zero).  Run at every
// sharded cost / linearize / refine call: the call is collective anyway, and a check only "after a change" would leave a rank
// that changed nothing out of the all-reduce.
static int32_t check_loss_agreement(lvba_visual_s *h)
{
    BlockSys &bs = h->bs;
    if (!bs.distributed()) return LVBA_OK;
    int64_t v[6];
    for (int f = 0; f < 2; ++f) {
        v[f] = h->loss_kind[f];
        memcpy(&v[2 + f], &h->loss_scale[f], sizeof v[0]); // scale >= 0: bits < 2^63, their negation does not overflow
    }
    v[4] = (int64_t)h->priors.size(); v[5] = prior_hash(h->priors);
    bool same[6];
    TRY(bs_ranks_agree(bs, v, 6, same));
    for (int e = 0; e < 4; ++e)
        if (!same[e]) return fail(LVBA_ERR_ARG, "the ranks of a sharded visual handle set different losses");
    for (int e = 4; e < 6; ++e)
        if (!same[e]) return fail(LVBA_ERR_ARG, "the ranks of a sharded visual handle set different camera priors");
    return LVBA_OK;
}

static bool loss_ok(const lvba_loss *l)
{
    if (!l || l->kind == LVBA_LOSS_TRIVIAL) return true;
    if (l->kind < LVBA_LOSS_TRIVIAL || l->kind > LVBA_LOSS_TUKEY) return false;
    return isfinite(l->scale) && l->scale > 0.0;
}

extern "C" int32_t lvba_visual_set_loss(lvba_visual_t h, const lvba_loss *reproj, const lvba_loss *plane)
{
    if (!h) return fail(LVBA_ERR_ARG, "NULL handle");
    if (!loss_ok(reproj)) return fail(LVBA_ERR_ARG, "reprojection loss: unknown kind %d or scale not finite and > 0", reproj->kind);
    if (!loss_ok(plane)) return fail(LVBA_ERR_ARG, "plane loss: unknown kind %d or scale not finite and > 0", plane->kind);
    const lvba_loss *ls[2] = {reproj, plane};
    for (int f = 0; f < 2; ++f) {
        const bool trivial = !ls[f] || ls[f]->kind == LVBA_LOSS_TRIVIAL;
        h->loss_kind[f] = trivial ? LVBA_LOSS_TRIVIAL : ls[f]->kind;
        h->loss_scale[f] = trivial ? 0.0 : ls[f]->scale;
    }
    return LVBA_OK;
}

// ------------------------------------------------------------------------------------------ camera pose priors
// The blocks that hold something besides priors: what the pair pass writes on one rank (a prior adds to those and writes the
// others); on a sharded handle the whole store is cleared before every linearisation, so every block is added to -- there the
// list is the union pattern the packed all-reduce carries (empty: the whole store travels).
static int32_t prior_pattern(lvba_visual_s *h)
{
    if (h->pat_known) return LVBA_OK;
    BlockSys &bs = h->bs;
    if (!bs.distributed() || bs.d_ar_slot) TRY(bs_pattern_slots(bs, h->pat_slots));
    h->pat_known = true;
    return LVBA_OK;
}

// h->priors -> the solver order, the scatter tables (those of the LiDAR stage, prior_tables.h) and their device copies
static int32_t bind_priors(lvba_visual_s *h)
{
    BlockSys &bs = h->bs;
    TRY(h->pt.release(bs));
    h->vp = VisPriorDev{};
    if (h->priors.empty()) return LVBA_OK;
    TRY(prior_pattern(h));
    TRY(h->pt.bind(bs, h->priors, h->pat_slots, bs.distributed(), 2, nullptr));
    h->vp.tab = h->pt.dev;
    h->vp.active = bs.rank == 0 ? 1 : 0; // the cameras are replicated over the ranks: one of them adds their priors
    h->vp.fixed_cam = bs.iperm[0];
    h->vp.pscal = h->d_pscal;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_set_priors(lvba_visual_t h, int32_t n, const lvba_prior *priors)
{
    if (!h) return fail(LVBA_ERR_ARG, "handle is NULL");
    TRY(prior_cap(n));
    TRY(prior_validate(n, priors, h->M));
    BlockSys &bs = h->bs;
    if (h->finalized) { // the store is laid out: every relative pair must be one of its blocks
        TRY(prior_pattern(h));
        // sharded: only the blocks of the union pattern travel
        TRY(prior_pairs_in_store(bs, n, priors, bs.d_ar_slot ? &h->pat_slots : nullptr, nullptr, "cameras", "linearize"));
    }
    std::vector<lvba_prior> old;
    old.swap(h->priors); // (old: what the handle held)
    prior_store(bs, h->finalized, n, priors, h->priors);
    if (!h->finalized) return LVBA_OK;
    const int32_t rc = bind_priors(h);
    if (rc != LVBA_OK) { // out of memory / a failed upload: the handle keeps the priors it had (their pairs are blocks of the store)
        h->priors.swap(old);
        bind_priors(h);
    }
    return rc;
}

extern "C" int32_t lvba_visual_prior_residuals(lvba_visual_t h, const double *q, const double *t, double *e, double *cost)
{
    if (!h || !q || !t) return fail(LVBA_ERR_ARG, "NULL argument");
    if (!h->finalized && h->bs.distributed()) // finalize is collective there; this call is not
        return fail(LVBA_ERR_STATE, "prior_residuals on a sharded handle must follow its first cost / linearize / refine call");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    const int64_t n = h->vp.tab.n;
    if (n == 0) { if (cost) *cost = 0.0; return LVBA_OK; }
    DevArr<double> d(bs.stream);
    HIPCHK(d.alloc((size_t)(6 * n + 1 + 7 * (int64_t)h->M)));
    double *de = d, *dq = de + 6 * n + 1, *dt = dq + 4 * (int64_t)h->M;
    lvba::hvec<double> st(7 * (size_t)h->M);
    for (int c = 0; c < h->M; ++c) {
        const int I = bs.iperm[c];
        for (int a = 0; a < 4; ++a) st[4 * (size_t)I + a] = q[4 * c + a];
        for (int a = 0; a < 3; ++a) st[4 * (size_t)h->M + 3 * (size_t)I + a] = t[3 * c + a];
    }
    HIPCHK(lvba::copy_h2d(dq, st.data(), st.size() * sizeof(double)));
    VisPriorDev vp = h->vp;
    vp.active = 1; // rank-local: every rank holds the cameras and the priors
    vprior_launch_trial(vp, nullptr, nullptr, nullptr, nullptr, dq, dt, de + 6 * n, nullptr, false, de, bs.stream);
    HIPCHK(hipGetLastError());
    double c2 = 0.0;
    if (e) HIPCHK(hipMemcpyAsync(e, de, (size_t)(6 * n) * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipMemcpyAsync(&c2, de + 6 * n, sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    if (cost) *cost = 0.5 * c2;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_dist_init(lvba_visual_t h, int32_t n_ranks, int32_t rank, const char uid[128])
{
    if (!h || !uid) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->finalized) return fail(LVBA_ERR_STATE, "dist_init must precede the first cost/linearize/refine call");
    return bs_dist_init(h->bs, n_ranks, rank, uid, nullptr);
}

extern "C" int32_t lvba_visual_dist_init_external(lvba_visual_t h, int32_t n_ranks, int32_t rank, lvba_allreduce_fn fn, void *ctx)
{
    if (!h || !fn) return fail(LVBA_ERR_ARG, "NULL argument");
    if (h->finalized) return fail(LVBA_ERR_STATE, "dist_init must precede the first cost/linearize/refine call");
    return bs_dist_init_external(h->bs, n_ranks, rank, fn, ctx, nullptr);
}

extern "C" int32_t lvba_visual_cost(lvba_visual_t h, const double *q, const double *t, const double *X, double *cost)
{
    if (!h || !q || !t || !X || !cost) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(check_loss_agreement(h));
    TRY(import_state(h, q, t, X));
    vis_launch_residuals(h->dev(), false, h->d_q, h->d_t, h->d_X, h->d_blkpart, h->d_scal, bs.stream);
    vprior_launch_trial(h->vp, nullptr, nullptr, nullptr, nullptr, h->d_q, h->d_t, h->d_scal, nullptr, true, nullptr, bs.stream);
    TRY(allreduce_scalars(h, 0, 1));
    HIPCHK(hipMemcpyAsync(h->h_pin, h->d_scal, sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    HIPCHK(hipGetLastError());
    *cost = 0.5 * h->h_pin[0];
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_info(lvba_visual_t h, lvba_balm_info_t *info)
{
    if (!h || !info) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    memset(info, 0, sizeof *info);
    info->n_poses = h->M; info->n_ranks = h->bs.n_ranks; info->n_voxels = h->Ta; info->n_voxels_global = h->Ta;
    info->n_factors = h->O; info->n_pairs = h->bs.Q; info->n_blocks = h->bs.nnzb; info->band_blocks = h->bs.Bb;
    info->use_band = h->bs.use_band ? 1 : 0; info->hess_bytes = h->bs.hblk_doubles * 8; info->device_bytes = h->bs.device_bytes;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_pair_layout(lvba_visual_t h, lvba_pair_layout_t *out, int64_t *item_len, int64_t *item_slot, int64_t cap)
{
    if (!h || !out) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    return bs_pair_layout(h->bs, out, item_len, item_slot, cap);
}

extern "C" int32_t lvba_visual_eval_layout(lvba_visual_t h, lvba_eval_layout_t *out)
{
    if (!h || !out) return fail(LVBA_ERR_ARG, "NULL argument");
    TRY(finalize(h));
    const VisDev d = h->dev();
    const VisEvalLayout l = vis_eval_layout(d);
    memset(out, 0, sizeof *out);
    out->slices = d.S; out->unit_form = l.cam_form; out->units = l.cam_units; out->unit_grid = l.cam_grid;
    out->point_groups = l.point_groups; out->back_groups = l.back_groups; out->point_grid = l.point_grid; out->back_grid = l.back_grid;
    out->n_groups = d.Ta; out->n_factors = d.O;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_residual_sq(lvba_visual_t h, const double *q, const double *t, const double *X, double *obs_sq,
                                           double *plane_sq)
{
    if (!h || !q || !t || !X || !obs_sq || !plane_sq) return fail(LVBA_ERR_ARG, "NULL argument");
    if (!h->finalized && h->bs.distributed()) // finalize is collective there; this call is not
        return fail(LVBA_ERR_STATE, "residual_sq on a sharded handle must follow its first cost / linearize / refine call");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(import_state(h, q, t, X));
    const int64_t n = h->O + h->Ta;
    lvba::hvec<double> hs((size_t)std::max<int64_t>(1, n));
    DevArr<double> ds(bs.stream);
    HIPCHK(ds.alloc((size_t)std::max<int64_t>(1, n)));
    vis_launch_residual_sq(h->dev(), h->d_q, h->d_t, h->d_X, ds, bs.stream);
    if (n) HIPCHK(hipMemcpyAsync(hs.data(), ds, ds.bytes((size_t)n), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    HIPCHK(hipGetLastError());
    for (int64_t o = 0; o < h->O_all; ++o) obs_sq[o] = NAN;     // observations of inactive landmarks
    for (int64_t i = 0; i < h->T; ++i) plane_sq[i] = NAN;
    for (int64_t o = 0; o < h->O; ++o) obs_sq[h->obs_src[o]] = hs[o];
    for (int64_t i = 0; i < h->Ta; ++i) plane_sq[h->act[i]] = hs[h->O + i];
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_linearize(lvba_visual_t h, const double *q, const double *t, const double *X, double radius,
                                         double *S, double *rhs, double *cost)
{
    if (!h || !q || !t || !X) return fail(LVBA_ERR_ARG, "NULL argument");
    if (!(radius > 0.0)) return fail(LVBA_ERR_ARG, "radius must be > 0");
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(check_loss_agreement(h));
    TRY(import_state(h, q, t, X));
    lvba_visual_opts o;
    lvba_visual_default_opts(&o);
    const VisDev d = h->dev();
    vis_launch_residuals(d, true, h->d_q, h->d_t, h->d_X, h->d_blkpart, h->d_scal, bs.stream);
    vprior_launch_lin0(h->vp, h->d_q, h->d_t, h->d_scal, bs.stream);
    TRY(allreduce_scalars(h, 0, 1));
    TRY(enqueue_colnorms(h));
    TRY(enqueue_reduced_system(h, radius, o));
    const int64_t n = 6 * (int64_t)h->M;
    DevArr<double> dS(bs.stream); // freed on every path, error returns included
    if (S) {
        HIPCHK(dS.alloc((size_t)(n * n)));
        launch_export_dense(bs.Hblk(), bs.Bb, h->M, bs.d_perm, dS, bs.stream);
        HIPCHK(hipMemcpyAsync(S, dS, dS.bytes((size_t)(n * n)), hipMemcpyDeviceToHost, bs.stream));
    }
    if (rhs) {
        launch_export_vec(bs.g(), bs.d_perm, h->M, h->d_out, bs.stream);
        HIPCHK(hipMemcpyAsync(rhs, h->d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    }
    HIPCHK(hipMemcpyAsync(h->h_pin, h->d_scal, sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    HIPCHK(hipGetLastError());
    if (cost) *cost = 0.5 * h->h_pin[0];
    h->have_lin = true;
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_solve(lvba_visual_t h, double *x, int32_t *solver)
{
    if (!h || !x) return fail(LVBA_ERR_ARG, "NULL argument");
    if (!h->finalized || !h->have_lin) return fail(LVBA_ERR_STATE, "lvba_visual_solve needs a prior lvba_visual_linearize");
    BlockSys &bs = h->bs;
    if (bs.distributed()) return fail(LVBA_ERR_STATE, "lvba_visual_solve is not available on a sharded handle");
    HIPCHK(hipSetDevice(bs.device));
    TRY(bs_enqueue_solve(bs, 0.0)); // the damping is in the system (the LM diagonal of the linearisation)
    launch_export_vec(bs.d_dx, bs.d_perm, h->M, h->d_out, bs.stream);
    HIPCHK(hipMemcpyAsync(x, h->d_out, (size_t)6 * h->M * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    int st = 0;
    HIPCHK(hipMemcpyAsync(&st, bs.d_status, sizeof(int), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    HIPCHK(hipGetLastError());
    if (solver) *solver = !bs.d_bcr ? 0 : bcr_block_scalars(bs.Bb) == 32 ? 1 : 2;
    if (st) return fail(LVBA_NUM_FACTORIZATION, "zero or non-positive pivot in the reduced camera solve");
    return LVBA_OK;
}

extern "C" int32_t lvba_visual_refine(lvba_visual_t h, double *q, double *t, double *X, const lvba_visual_opts *opts,
                                      lvba_visual_trace *trace, int32_t trace_cap, int32_t *n_trace, int32_t *termination)
{
    if (!h || !q || !t || !X) return fail(LVBA_ERR_ARG, "NULL argument");
    if (n_trace) *n_trace = 0;
    h->have_lin = false;
    TRY(finalize(h));
    BlockSys &bs = h->bs;
    HIPCHK(hipSetDevice(bs.device));
    TRY(check_loss_agreement(h));
    lvba_visual_opts o;
    if (opts) o = *opts; else lvba_visual_default_opts(&o);
    auto wall_us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tw0 = wall_us();
    TRY(import_state(h, q, t, X));
    const double tw1 = wall_us();
    int32_t rows = 0, term = LVBA_TERM_NO_CONVERGENCE, rc = LVBA_OK;
    auto push = [&](int it, int acc, int valid, double cost, double dc, double sn, double rad, double rho, double gm) {
        if (trace && rows < trace_cap) {
            lvba_visual_trace &r = trace[rows];
            r.iter = it; r.accepted = acc; r.valid = valid; r.reserved = 0; r.cost = cost; r.cost_change = dc; r.step_norm = sn;
            r.radius = rad; r.rho = rho; r.gradient_max_norm = gm;
        }
        rows++;
    };
    VisDev d = h->dev();
    // iteration 0: evaluate, fix the Jacobi scaling
    vis_launch_residuals(d, true, h->d_q, h->d_t, h->d_X, h->d_blkpart, h->d_scal, bs.stream);
    vprior_launch_lin0(h->vp, h->d_q, h->d_t, h->d_scal, bs.stream);
    TRY(allreduce_scalars(h, 0, 1));
    TRY(enqueue_colnorms(h));
    HIPCHK(hipMemcpyAsync(h->h_pin, h->d_scal, sizeof(double), hipMemcpyDeviceToHost, bs.stream));
    HIPCHK(hipStreamSynchronize(bs.stream));
    double cost = 0.5 * h->h_pin[0];
    const double tw2 = wall_us();
    double radius = o.initial_radius, decrease_factor = 2.0;
    bool first = true;
    int invalid_run = 0;
    if (!isfinite(cost)) { term = LVBA_TERM_FAILURE; rc = fail(LVBA_NUM_NONFINITE, "non-finite initial cost"); }
    // LVBA_TIMING=vis: HIP events between the phases of every iteration, averages on stderr at the end (tools/visual_bench.py)
    static const bool prof = timing_on("vis", true); // (a stream synchronisation per phase: only when asked for by name)
    constexpr int NPH = 6, PCAP = 64;
    std::vector<hipEvent_t> pev;
    int pn = 0;
    if (prof) {
        pev.resize((size_t)NPH * PCAP);
        for (auto &e : pev) hipEventCreate(&e);
    }
    auto mark = [&](int ph) { if (prof && pn < PCAP) hipEventRecord(pev[(size_t)pn * NPH + ph], bs.stream); };
    for (int it = 1; rc == LVBA_OK; ++it) {
        // linearised system at the current point (its gradient norm belongs to the row of the previous iteration)
        mark(0);
        TRY(enqueue_reduced_system(h, radius, o));
        mark(1);
        TRY(bs_enqueue_solve(bs, 0.0));
        mark(2);
        if (!bs.distributed()) {
            // one rank: back-substitution, candidate, its cost, and one closing kernel that sums the partial lists and writes what
            // the host reads below into the pinned buffer (no reductions of their own, no device-to-host copies)
            mark(3);
            vis_launch_step_and_trial(d, bs.d_dx, h->d_q, h->d_t, h->d_X, h->d_q2, h->d_t2, h->d_X2, h->d_blkpart, h->d_scal, h->d_gmax,
                                      bs.d_status, h->h_pin, bs.stream, &h->vp);
            mark(4);
        } else {
            vis_launch_back(d, bs.d_dx, h->d_q, h->d_t, h->d_X, h->d_blkpart, h->d_scal + 2, bs.stream);
            mark(3);
            vis_launch_apply(d, bs.d_dx, h->d_q, h->d_t, h->d_X, h->d_q2, h->d_t2, h->d_X2, h->d_blkpart, h->d_scal + 3, bs.stream);
            vis_launch_residuals(d, false, h->d_q2, h->d_t2, h->d_X2, h->d_blkpart, h->d_scal + 1, bs.stream);
            vprior_launch_trial(h->vp, h->d_q, h->d_t, bs.d_dx, h->d_sc_cam, h->d_q2, h->d_t2, h->d_scal + 1, h->d_scal + 2, true, nullptr,
                                bs.stream); // (one rank adds the priors' trial cost and model cost change)
            mark(4);
            TRY(allreduce_scalars(h, 1, 4)); // candidate cost, model cost change, |step|^2, |x|^2: sums over the track shards
            HIPCHK(hipMemcpyAsync(h->h_pin, h->d_scal, 5 * sizeof(double), hipMemcpyDeviceToHost, bs.stream));
            HIPCHK(hipMemcpyAsync(h->h_pin + 8, h->d_gmax, sizeof(unsigned long long), hipMemcpyDeviceToHost, bs.stream));
            HIPCHK(hipMemcpyAsync(h->h_pin + 9, bs.d_status, sizeof(int), hipMemcpyDeviceToHost, bs.stream));
        }
        mark(5);
        if (prof && pn < PCAP) ++pn;
        HIPCHK(hipStreamSynchronize(bs.stream));
        HIPCHK(hipGetLastError());
        double gmax;
        memcpy(&gmax, h->h_pin + 8, sizeof(double));
        int st = 0;
        memcpy(&st, h->h_pin + 9, sizeof(int));
        if (first) { push(0, 1, 1, cost, 0.0, 0.0, radius, 0.0, gmax); first = false; }
        // TrustRegionMinimizer::FinalizeIterationAndCheckIfMinimizerCanContinue: iterations, then gradient, then radius
        if (it > o.max_iter) { term = LVBA_TERM_NO_CONVERGENCE; break; }
        if (gmax <= o.gradient_tolerance) { term = LVBA_TERM_GRADIENT; break; }
        const double cand = 0.5 * h->h_pin[1], model = h->h_pin[2];
        const double step_norm = sqrt(h->h_pin[3]), x_norm = sqrt(h->h_pin[4]);
        const bool finite_step = st == 0 && isfinite(model) && isfinite(step_norm);
        if (!finite_step || !(model > 0.0)) { // LevenbergMarquardtStrategy::StepIsInvalid = StepRejected(0): /2, /4, /8 ...
            radius = radius / decrease_factor;
            decrease_factor *= 2.0;
            push(it, 0, 0, cost, 0.0, 0.0, radius, 0.0, gmax);
            if (++invalid_run >= 5) { term = LVBA_TERM_FAILURE; rc = fail(LVBA_NUM_FACTORIZATION, "5 consecutive invalid steps"); }
            if (radius < o.min_radius) { term = LVBA_TERM_RADIUS; break; }
            continue;
        }
        invalid_run = 0;
        if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) {
            push(it, 0, 1, cost, cost - cand, step_norm, radius, 0.0, gmax);
            term = LVBA_TERM_PARAMETER;
            break;
        }
        const double cost_change = cost - cand;
        if (fabs(cost_change) <= o.function_tolerance * cost) {
            push(it, 0, 1, cost, cost_change, step_norm, radius, 0.0, gmax);
            term = LVBA_TERM_FUNCTION;
            break;
        }
        const double rho = cost_change / model;
        if (isfinite(cand) && rho > o.min_relative_decrease) {
            // the accepted point becomes the current one: nothing to evaluate -- the kernels of the next iteration linearise from
            // the state itself (residuals and Jacobians are re-computed where they are used)
            std::swap(h->d_q, h->d_q2); std::swap(h->d_t, h->d_t2); std::swap(h->d_X, h->d_X2);
            cost = cand;
            radius = std::min(o.max_radius, radius / std::max(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0)));
            decrease_factor = 2.0;
            push(it, 1, 1, cost, cost_change, step_norm, radius, rho, gmax);
        } else {
            radius = radius / decrease_factor;
            decrease_factor *= 2.0;
            push(it, 0, 1, cand, cost_change, step_norm, radius, rho, gmax);
            if (radius < o.min_radius) { term = LVBA_TERM_RADIUS; break; }
        }
    }
    if (prof) {
        hipStreamSynchronize(bs.stream);
        double acc[NPH] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < pn; ++k)
            for (int ph = 0; ph + 1 < NPH; ++ph) {
                float ms = 0.f;
                hipEventElapsedTime(&ms, pev[(size_t)k * NPH + ph], pev[(size_t)k * NPH + ph + 1]);
                acc[ph] += ms;
            }
        for (int k = 0; k + 1 < pn; ++k) { // end of iteration k -> start of iteration k + 1: host turn-around + the accepted point's linearisation
            float ms = 0.f;
            hipEventElapsedTime(&ms, pev[(size_t)k * NPH + NPH - 1], pev[(size_t)(k + 1) * NPH]);
            acc[NPH - 1] += ms;
        }
        if (pn > 0)
            fprintf(stderr, "[lvba visual profile] %d iterations, us each: reduced system %.1f | solve %.1f | back %.1f | step + trial cost %.1f | "
                            "copies %.1f | between iterations %.1f\n", pn, 1e3 * acc[0] / pn, 1e3 * acc[1] / pn, 1e3 * acc[2] / pn,
                    1e3 * acc[3] / pn, 1e3 * acc[4] / pn, pn > 1 ? 1e3 * acc[5] / (pn - 1) : 0.0);
        for (auto &e : pev) hipEventDestroy(e);
    }
    if (n_trace) *n_trace = std::min(rows, trace_cap > 0 ? trace_cap : 0);
    if (termination) *termination = term;
    const double tw3 = wall_us();
    const int32_t rc2 = export_state(h, q, t, X);
    if (prof)
        fprintf(stderr, "[lvba visual profile] host clock, us: state upload %.0f | first evaluation + Jacobi scaling %.0f | iterations %.0f | state download %.0f\n",
                tw1 - tw0, tw2 - tw1, tw3 - tw2, wall_us() - tw3);
    return rc != LVBA_OK ? rc : rc2;
}
