// pose_graph.hip -- pose-graph relaxation over odometry and loop closures (lvba_posegraph_relax; the problem and the LM rule are in
// include/lvba_hip.h, the rule's code in lm_rule.h, the per-edge arithmetic in posegraph_device.h, both also compiled for the host
// by the tests).
//
// The edges are priors: N - 1 odometry steps, the caller's closures, one POSE prior on the anchor, in that order.  The assembly is
// the prior tables' (PriorTables::bind with all_add = false and no other slots: every off-diagonal block is written by edges
// only), the solve is bs_enqueue_solve on a BlockSys built from the edges alone (no factor groups).  Kernels of this file:
//   pg_odometry_kernel  a thread per step: Z0_i = X0_i^-1 X0_{i+1} and the rest of that edge's record, written into the record
//                       array the tables uploaded (the host fills only the indices of an odometry edge).
//   pg_zero_kernel      the diagonal blocks and g before an evaluation (the scatter adds to those; the others it writes).
//   pg_lin_kernel       a lane per edge: the lin record of priors.hip's layout, a closure's scaled by rho' (posegraph_device.h),
//                       and the three cost sums (all edges | odometry | closures) in the fixed order of prior_grid_sum.
//   pg_cost_kernel      the same sums at the trial point without Jacobians; at the result it also writes the closures' weights.
//   pg_report_kernel    one workgroup: max |dx|, and the iteration's numbers into pinned host memory (zero-copy).
// The retraction, the predicted decrease and the pose permutation are balm_kernels.hip's launchers.  No atomics on data: two calls
// give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_system.h"
#include "prior_tables.h"
#include "posegraph_device.h"
#include "lm_rule.h"

using namespace lvba;

namespace {

// edge classes by index: [0, n_odom) odometry, [n_odom, n_odom + n_clos) closures, then the anchor
struct PgEdges {
    PriorRec *pr;
    int32_t n, n_odom, n_clos;
    int32_t loss_kind;
    double loss_scale;
};

__global__ __launch_bounds__(256) void pg_odometry_kernel(PgEdges ed, const double *__restrict__ x0, double inv_sigma_rot, double inv_sigma_pos)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ed.n_odom) return;
    PriorRec &p = ed.pr[k];
    double Xi[12], Xj[12], meas[12], oi[12], oj[12], L[36];
    prior_load_pose(x0, p.I, Xi);
    prior_load_pose(x0, p.J, Xj);
    pg_odometry_record(Xi, Xj, inv_sigma_rot, inv_sigma_pos, meas, oi, oj, L);
#pragma unroll
    for (int a = 0; a < 12; ++a) { p.meas[a] = meas[a]; p.oi[a] = oi[a]; p.oj[a] = oj[a]; }
#pragma unroll
    for (int a = 0; a < 36; ++a) p.L[a] = L[a];
}

__global__ __launch_bounds__(256) void pg_zero_kernel(double *__restrict__ Hblk, double *__restrict__ g, int32_t N, int64_t Bb1)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < 36 * (int64_t)N) Hblk[(t / 36) * Bb1 * 36 + t % 36] = 0.0;
    else if (t < 42 * (int64_t)N) g[t - 36 * (int64_t)N] = 0.0;
}

template <int KIND>
__device__ __forceinline__ double pg_lin_one(const PriorRec &p, const double *__restrict__ poses, int loss_kind, double loss_scale,
                                             double *__restrict__ o, double *w)
{
    double Ti[12], Tj[12];
    prior_load_pose(poses, p.I, Ti);
    if (KIND == PRIOR_RELATIVE) prior_load_pose(poses, p.J, Tj);
    return pg_edge_lin(KIND, p.meas, p.oi, p.oj, p.L, Ti, Tj, p.flip != 0, loss_kind, loss_scale, o, w);
}

// sums [3]: all edges | odometry | closures
__global__ __launch_bounds__(64) void pg_lin_kernel(PgEdges ed, const double *__restrict__ poses, double *__restrict__ lin,
                                                    double *__restrict__ part, unsigned *__restrict__ ticket, double *__restrict__ sums)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c = 0.0, co = 0.0, cc = 0.0, w;
    if (k < ed.n) {
        const PriorRec &p = ed.pr[k];
        double *o = lin + PL_LIN * (int64_t)k;
        if (k < ed.n_odom) c = co = pg_lin_one<PRIOR_RELATIVE>(p, poses, VLOSS_TRIVIAL, 0.0, o, &w);
        else if (k < ed.n_odom + ed.n_clos) c = cc = pg_lin_one<PRIOR_RELATIVE>(p, poses, ed.loss_kind, ed.loss_scale, o, &w);
        else c = pg_lin_one<PRIOR_POSE>(p, poses, VLOSS_TRIVIAL, 0.0, o, &w);
    }
    prior_grid_sum<3>({c, co, cc}, part, ticket, {sums, sums + 1, sums + 2}, false);
}

// weight [n_clos] or null
__global__ __launch_bounds__(64) void pg_cost_kernel(PgEdges ed, const double *__restrict__ poses, double *__restrict__ part,
                                                     unsigned *__restrict__ ticket, double *__restrict__ sums, double *__restrict__ weight)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    double c = 0.0, co = 0.0, cc = 0.0;
    if (k < ed.n) {
        const PriorRec &p = ed.pr[k];
        const bool clos = k >= ed.n_odom && k < ed.n_odom + ed.n_clos;
        double Ti[12], Tj[12], w;
        prior_load_pose(poses, p.I, Ti);
        if (p.kind == PRIOR_RELATIVE) prior_load_pose(poses, p.J, Tj);
        c = pg_edge_cost(p.kind, p.meas, p.oi, p.oj, p.L, Ti, Tj, clos ? ed.loss_kind : VLOSS_TRIVIAL, ed.loss_scale, &w);
        if (k < ed.n_odom) co = c;
        if (clos) {
            cc = c;
            if (weight) weight[k - ed.n_odom] = w;
        }
    }
    prior_grid_sum<3>({c, co, cc}, part, ticket, {sums, sums + 1, sums + 2}, false);
}

// sc: [0..2] sums at the current point, [3..5] at the trial point, [6] q1.  pin: [0..2] trial sums, [3] q1, [4..6] current sums,
// [7] the solve's status, [8] max |dx|
__global__ __launch_bounds__(256) void pg_report_kernel(const double *__restrict__ sc, const double *__restrict__ dx, int64_t n,
                                                        const int *__restrict__ status, double *__restrict__ pin)
{
    __shared__ double red[256];
    double m = 0.0;
    for (int64_t a = threadIdx.x; a < n; a += 256) m = fmax(m, fabs(dx[a])); // (fmax drops a NaN: a flagged solve is seen in status)
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pin[0] = sc[3]; pin[1] = sc[4]; pin[2] = sc[5]; pin[3] = sc[6];
        pin[4] = sc[0]; pin[5] = sc[1]; pin[6] = sc[2];
        pin[7] = (double)status[0];
        pin[8] = red[0];
        __threadfence_system();
    }
}

bool sigma_ok(double v) { return std::isfinite(v) && v > 0.0; }

// what the call owns on the device; released on every path
struct PgState {
    BlockSys bs;
    PriorTables pt;
    bool bs_on = false;
    double *pin = nullptr;
    std::vector<void *> mem;
    ~PgState()
    {
        if (bs_on) {
            (void)hipSetDevice(bs.device);
            if (bs.stream) (void)hipStreamSynchronize(bs.stream);
        }
        pt.free_mem();
        for (void *p : mem) DevicePool::get().free(p);
        if (pin) PinnedCache::get().release(pin);
        if (bs_on) bs_destroy(bs);
    }
    template <typename T> int32_t dmalloc(T **p, int64_t count)
    {
        TRY(bs_dmalloc(bs, p, count));
        mem.push_back(*p);
        return LVBA_OK;
    }
};

} // namespace

extern "C" void lvba_posegraph_default_opts(lvba_posegraph_opts *o)
{
    if (!o) return;
    *o = lvba_posegraph_opts{};
    o->anchor = 0; o->max_iter = 50;
    o->odom_sigma_rot = 0.01; o->odom_sigma_pos = 0.05;
    o->anchor_sigma_rot = 1e-4; o->anchor_sigma_pos = 1e-4;
    o->rel_tol = 1e-6;
    o->closure_loss = lvba_loss{LVBA_LOSS_TRIVIAL, 0, 0.0};
}

extern "C" int32_t lvba_posegraph_relax(int32_t n_poses, const double *poses, int32_t n_edges, const lvba_prior *edges,
                                        const lvba_posegraph_opts *opts, int32_t device, double *poses_out, double *edge_weight,
                                        lvba_lm_trace *trace, int32_t *n_trace, lvba_posegraph_report *report)
{
    if (!poses || !poses_out || !report || n_poses < 2 || n_edges < 0 || (n_edges > 0 && !edges))
        return lvba_fail(LVBA_ERR_ARG, "lvba_posegraph_relax: a null required pointer, n_poses %d < 2 or n_edges %d < 0", n_poses, n_edges);
    lvba_posegraph_opts o;
    lvba_posegraph_default_opts(&o);
    if (opts) o = *opts;
    if (!sigma_ok(o.odom_sigma_rot) || !sigma_ok(o.odom_sigma_pos) || !sigma_ok(o.anchor_sigma_rot) || !sigma_ok(o.anchor_sigma_pos) ||
        !sigma_ok(o.rel_tol) || o.max_iter < 0)
        return lvba_fail(LVBA_ERR_ARG, "lvba_posegraph_relax: sigmas and rel_tol must be finite and > 0, max_iter >= 0");
    if (o.anchor < 0 || o.anchor >= n_poses) return lvba_fail(LVBA_ERR_ARG, "lvba_posegraph_relax: anchor %d outside [0,%d)", o.anchor, n_poses);
    TRY(loss_validate(&o.closure_loss, "lvba_posegraph_relax"));
    const int32_t N = n_poses, K = n_edges;
    TRY(prior_cap(K));
    for (int32_t k = 0; k < K; ++k)
        if (edges[k].kind != LVBA_PRIOR_RELATIVE) return lvba_fail(LVBA_ERR_ARG, "edge %d: kind %d is not LVBA_PRIOR_RELATIVE", k, edges[k].kind);
    TRY(prior_validate(K, edges, N));
    lvba_prior anchor_prior;
    memset(&anchor_prior, 0, sizeof anchor_prior);
    anchor_prior.kind = LVBA_PRIOR_POSE;
    for (int32_t i = 0; i < N; ++i) { // a pose passes what a POSE prior's measurement passes (prior_tables.hip)
        anchor_prior.i = i;
        memcpy(anchor_prior.meas, poses + 12 * (size_t)i, sizeof anchor_prior.meas);
        if (prior_validate(1, &anchor_prior, N) != LVBA_OK) return lvba_fail(LVBA_ERR_ARG, "pose %d: non-finite, or its rotation is not orthonormal", i);
    }
    lvba_posegraph_report rep{};
    rep.solver_kind = -1;
    if (K == 0) { // nothing pulls: the odometry and the anchor are at rest at the input
        if (poses_out != poses) memcpy(poses_out, poses, 96 * (size_t)N);
        if (n_trace) *n_trace = 0;
        *report = rep;
        return LVBA_OK;
    }
    TRY(check_device(device));

    // ---- the edges as priors: odometry (indices only; pg_odometry_kernel writes the rest on the device), closures, anchor
    const int32_t n_odom = N - 1, E = n_odom + K + 1;
    std::vector<lvba_prior> all((size_t)E);
    memset(all.data(), 0, all.size() * sizeof(lvba_prior));
    for (int32_t i = 0; i < n_odom; ++i) { all[(size_t)i].kind = LVBA_PRIOR_RELATIVE; all[(size_t)i].i = i; all[(size_t)i].j = i + 1; }
    for (int32_t k = 0; k < K; ++k) { all[(size_t)(n_odom + k)] = edges[k]; all[(size_t)(n_odom + k)].reserved = 0; }
    anchor_prior.i = o.anchor;
    memcpy(anchor_prior.meas, poses + 12 * (size_t)o.anchor, sizeof anchor_prior.meas);
    for (int a = 0; a < 6; ++a) anchor_prior.sqrt_info[7 * a] = 1.0 / (a < 3 ? o.anchor_sigma_rot : o.anchor_sigma_pos);
    all[(size_t)(E - 1)] = anchor_prior;

    PgState st;
    BlockSys &bs = st.bs;
    st.bs_on = true;
    TRY(bs_init(bs, device));
    for (int32_t k = 0; k < E - 1; ++k) { bs.edge_i.push_back(all[(size_t)k].i); bs.edge_j.push_back(all[(size_t)k].j); }
    {   // a system without factor groups: G = 0, F = Q = 0.  bs_build then sizes every list from the edges (band, ordering, dissection
        // plan) and from N; its group passes (adjacency, pose-major order, pair lists) skip their launches for F = Q = 0, and this
        // file never runs the pair pass or the factor pass, whose grids would be empty.
        const int64_t voff0 = 0;
        TRY(bs_build(bs, N, 0, &voff0, nullptr));
    }
    rep.solver_kind = bs.nd.active ? LVBA_PG_SOLVER_DISSECTED : bs.use_band ? LVBA_PG_SOLVER_BAND : LVBA_PG_SOLVER_DENSE;
    TRY(st.pt.bind(bs, all, lvba::hvec<int64_t>(), false, 3, nullptr));
    const PriorDev &pd = st.pt.dev;
    const hipStream_t s = bs.stream;
    PgEdges ed;
    ed.pr = const_cast<PriorRec *>(pd.pr); ed.n = E; ed.n_odom = n_odom; ed.n_clos = K;
    ed.loss_kind = o.closure_loss.kind; ed.loss_scale = o.closure_loss.kind == LVBA_LOSS_TRIVIAL ? 1.0 : o.closure_loss.scale;

    double *d_io = nullptr, *d_x0 = nullptr, *d_cur = nullptr, *d_trial = nullptr, *d_sc = nullptr, *d_w = nullptr;
    TRY(st.dmalloc(&d_io, 12 * (int64_t)N)); TRY(st.dmalloc(&d_x0, 12 * (int64_t)N)); TRY(st.dmalloc(&d_cur, 12 * (int64_t)N));
    TRY(st.dmalloc(&d_trial, 12 * (int64_t)N)); TRY(st.dmalloc(&d_sc, 8)); TRY(st.dmalloc(&d_w, K));
    HIPCHK(PinnedCache::get().acquire((void **)&st.pin, 4096));
    double *pin = st.pin;
    HIPCHK(hipMemsetAsync(d_sc, 0, 8 * sizeof(double), s));
    HIPCHK(copy_h2d(d_io, poses, 96 * (size_t)N));
    launch_import_poses(d_io, bs.d_perm, N, d_x0, s);
    HIPCHK(hipMemcpyAsync(d_cur, d_x0, 96 * (size_t)N, hipMemcpyDeviceToDevice, s));
    pg_odometry_kernel<<<(unsigned)((n_odom + 255) / 256), 256, 0, s>>>(ed, d_x0, 1.0 / o.odom_sigma_rot, 1.0 / o.odom_sigma_pos);
    HIPCHK(hipGetLastError());

    const unsigned egrid = (unsigned)((E + 63) / 64);
    const int64_t Bb1 = (int64_t)bs.Bb + 1, n6 = 6 * (int64_t)N;
    double cost_first = 0.0, max_step = 0.0;
    int32_t accepted = 0, worst = LVBA_OK;
    LmRule lm;
    lm.begin(0.01, 2.0, o.max_iter);
    std::vector<lvba_lm_trace> tr;
    while (!lm.done) {
        if (lm.evaluate) {
            pg_zero_kernel<<<(unsigned)((42 * (int64_t)N + 255) / 256), 256, 0, s>>>(bs.Hblk(), bs.g(), N, Bb1);
            pg_lin_kernel<<<egrid, 64, 0, s>>>(ed, d_cur, pd.lin, pd.part, pd.ticket, d_sc);
            launch_prior_scatter(pd, bs.Hblk(), bs.g(), s);
            HIPCHK(hipGetLastError());
            if (lm.iter == 0) { // the first cost decides whether anything runs at all
                HIPCHK(hipMemcpyAsync(pin + 4, d_sc, sizeof(double), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                cost_first = pin[4];
                if (!std::isfinite(cost_first)) return lvba_fail(LVBA_NUM_NONFINITE, "lvba_posegraph_relax: non-finite cost at the input poses");
                if (cost_first == 0.0) break;
            }
        }
        TRY(bs_enqueue_solve(bs, lm.u));
        launch_retract(d_cur, bs.d_dx, d_trial, N, s);
        launch_predicted_decrease(bs.Hblk(), bs.Bb, bs.g(), bs.d_dx, lm.u, n6, d_sc + 6, s);
        pg_cost_kernel<<<egrid, 64, 0, s>>>(ed, d_trial, pd.part, pd.ticket, d_sc + 3, nullptr);
        pg_report_kernel<<<1, 256, 0, s>>>(d_sc, bs.d_dx, n6, bs.d_status, pin);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        // the plain sums; a rejected row does not stop the loop (the header's rule: q / C1 < rel_tol on acceptance)
        const lvba_lm_trace row = lm.step(pin[4], pin[0], pin[3], pin[7] != 0.0, o.rel_tol, o.max_iter, false);
        tr.push_back(row);
        worst = std::max(worst, row.status);
        if (row.accepted) {
            std::swap(d_cur, d_trial);
            ++accepted;
            max_step = pin[8];
        }
    }
    const int32_t rows = (int32_t)tr.size();
    // ---- the result: the sums and the closures' weights at it, the poses in the caller's order
    pg_cost_kernel<<<egrid, 64, 0, s>>>(ed, d_cur, pd.part, pd.ticket, d_sc + 3, d_w);
    launch_export_poses(d_cur, bs.d_perm, N, d_io, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pin + 16, d_sc + 3, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> h_out(12 * (size_t)N), h_w((size_t)K);
    HIPCHK(copy_d2h(h_out.data(), d_io, 96 * (size_t)N));
    HIPCHK(copy_d2h(h_w.data(), d_w, 8 * (size_t)K));
    if (o.max_iter == 0) cost_first = pin[16];
    // everything has run: only now is anything of the caller's written
    rep.iterations = rows; rep.accepted = accepted; rep.status = worst;
    rep.cost_first = cost_first; rep.cost_last = pin[16]; rep.odom_cost_last = pin[17]; rep.closure_cost_last = pin[18];
    rep.max_step_last = max_step;
    memcpy(poses_out, h_out.data(), 96 * (size_t)N);
    if (edge_weight) memcpy(edge_weight, h_w.data(), 8 * (size_t)K);
    if (trace) std::copy(tr.begin(), tr.end(), trace);
    if (n_trace) *n_trace = rows;
    *report = rep;
    if (worst == LVBA_NUM_FACTORIZATION) return lvba_fail(worst, "lvba_posegraph_relax: zero or non-finite pivot in LDL^T");
    if (worst == LVBA_NUM_NONFINITE) return lvba_fail(worst, "lvba_posegraph_relax: non-finite cost");
    return LVBA_OK;
}
