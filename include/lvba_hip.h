/* lvba_hip.h -- C-ABI of liblvba_hip.so: the MI355X (gfx950) replacement for the LM-refinement
 * hot path of xuankuzcr/Global-LVBA.  Plain pointers and sizes only; no C++/torch types.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   lvba_balm_cost     <- BALM2::only_residual            include/BALM/bavoxel.hpp:641-648
 *                         (VOX_HESS::evaluate_only_residual  bavoxel.hpp:176-203)
 *   lvba_balm_eval     <- BALM2::divide_thread            include/BALM/bavoxel.hpp:597-639
 *                         (VOX_HESS::acc_evaluate2           bavoxel.hpp:68-174)
 *   lvba_balm_refine   <- BALM2::damping_iter             include/BALM/bavoxel.hpp:662-767
 *                         call sites src/lvba_system.cpp:264 (window BA) and :386 (global BA)
 *   lvba_balm_create   <- VOX_HESS::push_voxel / plvec_voxels (bavoxel.hpp:35,45-54): the packed
 *                         CSR copy of every admitted voxel's non-empty PointCluster slots
 *   lvba_balm_dist_*   <- the 16-way thread sum of bavoxel.hpp:626-633, as an RCCL all-reduce
 * The reference has no refine() symbol (SURVEY.md "five facts" #1); refine here is the name
 * BASELINE.json uses for damping_iter.
 *
 * Conventions (kept from the reference):
 *   pose      = T_world<-body, 12 doubles: R row-major (9) then p (3)          tools.hpp:147-207
 *   tangent   = [dtheta(3), dp(3)] per pose; retraction R*Exp(dtheta), p+dp   bavoxel.hpp:722-727
 *   cluster   = 10 doubles: Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz n  (P = sum p p^T, v = sum p, n = #points,
 *               body frame)                                                     tools.hpp:407-466
 *   factor    = one non-empty (voxel, pose) cluster slot; a voxel needs >= 2   bavoxel.hpp:45-54
 *   cost      = sum over voxels of lambda_min(cov of the merged, transformed clusters); the *_avg
 *               variants divide by the number of voxels (AVG_THR, bavoxel.hpp:11,634-635)
 *   H, g      = exact Hessian / gradient of the (un-averaged) cost, 6N x 6N / 6N
 *
 * Ownership: create() copies and repacks everything it is given onto the device; caller memory is
 * never referenced after a call returns.  The caller owns pose arrays and output buffers.
 * Threading: one caller thread per handle; calls are synchronous.  Handles are independent.
 * Errors: 0 = ok, < 0 = usage/runtime error, > 0 = numerical condition; never throws.
 * lvba_last_error() returns a thread-local message for the last non-zero status.
 * All arithmetic is IEEE fp64.  There is no CPU fallback: without a HIP device every entry point
 * that needs one returns LVBA_ERR_DEVICE.
 */
#ifndef LVBA_HIP_H
#define LVBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVBA_OK 0
#define LVBA_ERR_ARG (-1)          /* bad argument / shape */
#define LVBA_ERR_DEVICE (-2)       /* HIP runtime error or no device */
#define LVBA_ERR_NOMEM (-3)
#define LVBA_ERR_UNSUPPORTED (-4)
#define LVBA_ERR_DIST (-5)         /* RCCL error */
#define LVBA_ERR_STATE (-6)        /* call sequence error (e.g. lm_step before lm_begin) */
#define LVBA_NUM_FACTORIZATION 1   /* zero / non-finite pivot in LDL^T (reference: unchecked, bavoxel.hpp:707) */
#define LVBA_NUM_NONFINITE 2       /* non-finite cost */

typedef struct lvba_balm_s *lvba_balm_t;

/* LM options; lvba_balm_default_opts fills the reference's hard-coded values. */
typedef struct {
    int32_t max_iter;   /* 10   bavoxel.hpp:686 (rejected steps count) */
    int32_t reserved;
    double u0;          /* 0.01 bavoxel.hpp:664 */
    double v0;          /* 2    bavoxel.hpp:664 */
    double rel_tol;     /* 1e-6 bavoxel.hpp:760 */
} lvba_balm_opts;

/* One LM iteration, the quantities of the commented printf at bavoxel.hpp:737. */
typedef struct {
    int32_t iter;
    int32_t accepted;    /* q > 0 */
    int32_t evaluated;   /* H/g recomputed at the start of this iteration (is_calc_hess) */
    int32_t status;      /* LVBA_OK or LVBA_NUM_* for this iteration */
    double residual1;    /* averaged cost at the current poses */
    double residual2;    /* averaged cost at the trial poses */
    double u, v;         /* damping state used for this solve */
    double q;            /* residual1 - residual2 */
    double q1;           /* predicted decrease, averaged */
} lvba_lm_trace;

typedef struct {
    int32_t n_poses;
    int32_t n_ranks;
    int64_t n_voxels;        /* local shard */
    int64_t n_voxels_global;
    int64_t n_factors;       /* local shard */
    int64_t n_pairs;         /* local pose-pair contributions, sum k(k-1)/2 */
    int64_t n_chunks;        /* workgroup work items */
    int64_t n_blocks;        /* off-diagonal pose blocks (I>J) with at least one contributing voxel */
    int32_t band_blocks;     /* pose-block half bandwidth after ordering */
    int32_t use_band;        /* 1 = band LDL^T, 0 = dense */
    int64_t hess_bytes;      /* block-band Hessian storage */
    int64_t device_bytes;    /* total device memory held by the handle */
    int64_t allreduce_bytes; /* bytes all-reduced per evaluation (0 without a communicator): the union-pattern blocks + g + cost */
    int32_t twist_panels;    /* band solver: 64-column panels each END eliminates (0: plain top-down factorisation) */
    int32_t solve_ranks;     /* ranks the factorisation is spread over: 2 when ranks 0 and 1 take one end each, else 1 */
    int32_t trial_linearised; /* 1: the LM loop costs its trial point with the voxel pass of the evaluation (cost + voxel records),
                               * and an accepted step's next evaluation starts from those records (LiDAR handles only: 0 in
                               * lvba_visual_info) */
    int32_t y_fp32;           /* 1: LVBA_Y32=1 took effect -- the per-factor Y records travel as fp32 between the factor and the
                               * pair pass (an experiment: off-diagonal pose blocks then carry ~1e-7 relative rounding) */
    /* The damped solve by one level of nested dissection (csrc/nd_plan.h, csrc/ldlt_nd.h) instead of one band: a co-visibility
     * graph with a hub (a place crossed many times), or a long band on several ranks.  nd_kind 0: no (band / dense as above). */
    int32_t nd_kind;          /* 1: hub separator, 2: chunks of the band ordering */
    int32_t nd_arcs;          /* independent band systems (over all ranks) */
    int32_t nd_sep_poses;     /* poses of the separator system */
    int32_t nd_sep_band_blocks; /* its pose-block half bandwidth */
    double nd_model_band_ms, nd_model_nd_ms; /* the plan's cost model: seconds -> ms per solve, band against dissection */
} lvba_balm_info_t;

/* Accumulated device times (HIP events on the handle's stream) since the last reset, ms. */
typedef struct {
    double cost_ms;     int64_t cost_calls;      /* cost-only kernel (+ reduction) */
    double eval_ms;     int64_t eval_calls;      /* H/g/cost evaluation kernels */
    double solve_ms;    int64_t solve_calls;     /* damped LDL^T + triangular solves */
    double reduce_ms;   int64_t reduce_calls;    /* RCCL all-reduce */
    double cost_kernel_ms;  /* dominant kernel only: balm_cost_kernel */
    double eval_kernel_ms;  /* dominant kernel only: balm_eval_kernel */
} lvba_prof_t;

int32_t lvba_version(void);
const char *lvba_last_error(void);
int32_t lvba_device_count(void);

void lvba_balm_default_opts(lvba_balm_opts *opts);

/* Contiguous voxel range of rank r of G: [floor(V*r/G), floor(V*(r+1)/G)), the formula of
 * bavoxel.hpp:621-624 with thread -> GPU. */
void lvba_shard_range(int64_t n_voxels, int32_t rank, int32_t n_ranks, int64_t *head, int64_t *end);

/* Pack a problem (or one rank's voxel shard of it) onto HIP device `device`.
 *   voxel_off [n_voxels+1]  CSR offsets into pose_idx/clusters (voxel_off[0] may be non-zero: the
 *                           arrays are indexed by voxel_off[v]-voxel_off[0])
 *   pose_idx  [F]           observing pose of each factor, in [0, n_poses), distinct inside a voxel
 *   clusters  [F][10]
 * Every voxel must have >= 2 factors (push_voxel's admission rule). */
int32_t lvba_balm_create(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off,
                         const int32_t *pose_idx, const double *clusters, int32_t device,
                         lvba_balm_t *out);
/* The same with the clusters [F][10] already on `device` (a hipMalloc'ed / HIP-visible pointer, indexed like the host array
 * relative to voxel_off[0]): what the voxel front-end of this library hands over without a host round trip, and what a caller
 * that builds its clusters on the GPU would use.  voxel_off / pose_idx stay host arrays.  The device array is only read during
 * the call. */
int32_t lvba_balm_create_dev(int32_t n_poses, int64_t n_voxels, const int64_t *voxel_off, const int32_t *pose_idx,
                             const double *d_clusters, int32_t device, lvba_balm_t *out);
int32_t lvba_balm_destroy(lvba_balm_t h);

/* Optional, before the first cost/eval/refine call: pose ordering for the linear solver
 * (1 = reverse Cuthill-McKee on the pose co-visibility graph [default], 0 = caller order) and the
 * band/dense switch: the band LDL^T is used when (half-bandwidth + 128) < band_frac * 6N
 * (default 0.6), otherwise the dense one.  Results do not depend on either beyond rounding. */
int32_t lvba_balm_configure(lvba_balm_t h, int32_t ordering, double band_frac);
int32_t lvba_balm_info(lvba_balm_t h, lvba_balm_info_t *info);

/* Read-only view of how the pair pass (the off-diagonal pose blocks -sum Y_i Y_j^T) was laid out for this handle: which kernel
 * runs and the work items it walks.  An item is a run of pairs of one block (of one voxel window, when the lists are windowed),
 * cut at `cut` pairs; a block made of several items is summed from partial blocks afterwards. */
typedef struct {
    int32_t form;           /* 0: 16-lane kernel, 1: column-per-lane kernel, 2: column-per-lane kernel on fp32 records (LVBA_Y32=1) */
    int32_t cut;            /* longest item the lists were cut for, pairs */
    int64_t n_items;        /* work items */
    int64_t n_multi;        /* blocks summed from several partial blocks */
    int64_t n_partial;      /* partial blocks (= items that do not write their block directly) */
    int64_t window_voxels;  /* voxels per window of the lists; 0: not windowed */
    int64_t longest_item;   /* pairs */
    int64_t longest_multi;  /* most partial blocks summed into one block */
} lvba_pair_layout_t;
/* item_len / item_slot (both or either may be NULL; capacity `cap` >= n_items entries otherwise -- size them with a first call):
 * every item's pair count and destination in item order, a slot J * (band_blocks + 1) + (I - J) of the block-band store in the
 * SOLVER's pose order (I > J), or -1 - k for partial block k. */
int32_t lvba_balm_pair_layout(lvba_balm_t h, lvba_pair_layout_t *out, int64_t *item_len, int64_t *item_slot, int64_t cap);

/* Read-only view of how the evaluation kernels in front of the pair pass are launched for this handle: what the launchers use,
 * taken from the place they take it from.  A unit is one (pose or camera, slice) pair: every pose's / camera's list of factors /
 * observations is cut into `slices` pieces (LVBA_SLICES=1..64 replaces the rule's count).  Fields that do not apply to a stage
 * are 0. */
typedef struct {
    int32_t slices;         /* S: slices per pose (LiDAR) or camera (visual) */
    int32_t unit_form;      /* 0: one workgroup per unit; 1: one wavefront per unit, four units per workgroup (visual stage, short
                               slices; LVBA_VIS_CAM_FORM=0|1 replaces the rule's choice) */
    int64_t units;          /* n_poses * slices */
    int64_t unit_grid;      /* workgroups of the factor pass (LiDAR) / the camera kernel (visual) */
    int32_t point_groups;   /* visual: groups of 64 landmarks a workgroup of the landmark kernel walks, ... */
    int32_t back_groups;    /* ... and of the back-substitution */
    int64_t point_grid;     /* visual: workgroups of the landmark kernel, ... */
    int64_t back_grid;      /* ... and of the back-substitution */
    int64_t n_groups;       /* voxels (LiDAR) / landmarks with a plane (visual) */
    int64_t n_factors;      /* factors (LiDAR) / observations of those landmarks (visual) */
    int64_t n_chunks;       /* LiDAR: chunks of the voxel pass */
} lvba_eval_layout_t;
int32_t lvba_balm_eval_layout(lvba_balm_t h, lvba_eval_layout_t *out);

/* only_residual: cost at `poses` [N][12]; is_avg divides by the (global) voxel count. */
int32_t lvba_balm_cost(lvba_balm_t h, const double *poses, int32_t is_avg, double *cost);

/* divide_thread: H [6N*6N] (symmetric, so row/col-major agree), g [6N], averaged cost.
 * H and g may be NULL (kept on the device for lvba_balm_solve). */
int32_t lvba_balm_eval(lvba_balm_t h, const double *poses, double *H, double *g, double *cost_avg);

/* The same evaluation with H in SPARSE form, for problems whose dense matrix does not fit (10 000 poses: 28.8 GB): the
 * STRUCTURALLY non-zero 6x6 pose blocks of the lower triangle in the CALLER's pose order -- bi[k] >= bj[k], every unordered pose
 * pair that shares a voxel once (on a voxel shard without a union pattern: every slot of the band), the diagonal blocks in full
 * --, blocks[k][6 r + c] = H[6 bi[k] + r][6 bj[k] + c].  The set does not depend on the poses: it is the same on every call (the
 * sizing call and the filling call agree), and a block of it may be numerically zero.  *n_blocks receives the number of blocks;
 * call with capacity 0 (arrays may be NULL) to size the arrays.  g [6 n_poses] and cost_avg may be NULL. */
int32_t lvba_balm_eval_blocks(lvba_balm_t h, const double *poses, int64_t capacity, int32_t *bi, int32_t *bj, double *blocks,
                              int64_t *n_blocks, double *g, double *cost_avg);

/* Solve (H + u*diag(H)) dx = -g with the H, g of the last lvba_balm_eval (bavoxel.hpp:692-710). */
int32_t lvba_balm_solve(lvba_balm_t h, double u, double *dx);

/* damping_iter: refines poses in place.  trace may be NULL; at most opts->max_iter rows. */
int32_t lvba_balm_refine(lvba_balm_t h, double *poses_inout, const lvba_balm_opts *opts,
                         lvba_lm_trace *trace, int32_t *n_trace);

/* The same loop, one iteration per call (what bench.py times).  *done is set when the reference
 * loop would exit (max_iter reached or the bavoxel.hpp:760 test). */
int32_t lvba_balm_lm_begin(lvba_balm_t h, const double *poses, const lvba_balm_opts *opts);
int32_t lvba_balm_lm_step(lvba_balm_t h, lvba_lm_trace *row, int32_t *done);
int32_t lvba_balm_lm_end(lvba_balm_t h, double *poses_out);

/* Several INDEPENDENT refinements in one handle, advanced in lock-step -- the windows of LvbaSystem::runWindowBA
 * (src/lvba_system.cpp:232-302: one damping_iter per window, one after the other).  Group k owns the poses
 * [pose_off[k], pose_off[k+1]) and the voxels [voxel_off[k], voxel_off[k+1]); every factor of its voxels must be seen from
 * one of its poses.  The Hessian is block diagonal, so ONE evaluation, ONE band factorisation (damping per group) and ONE
 * cost pass per LM iteration serve all groups, while each group keeps the LM state of damping_iter (u, v, accept / reject,
 * the bavoxel.hpp:760 exit) for itself: group k's poses are what lvba_balm_refine gives for group k alone, up to rounding.
 *   lvba_balm_set_groups     after lvba_balm_create, before the first cost / eval / refine call (single rank only)
 *   lvba_balm_refine_groups  n_iter / status / cost_first / cost_last [n_groups] may be NULL; status[k] = LVBA_OK or
 *                            LVBA_NUM_NONFINITE.  Returns LVBA_NUM_FACTORIZATION (poses untouched) if a pivot of the joint
 *                            factorisation broke down: the groups are not independent then, refine them one by one. */
int32_t lvba_balm_set_groups(lvba_balm_t h, int32_t n_groups, const int32_t *pose_off, const int64_t *voxel_off);
int32_t lvba_balm_refine_groups(lvba_balm_t h, double *poses_inout, const lvba_balm_opts *opts, int32_t *n_iter,
                                int32_t *status, double *cost_first, double *cost_last);

/* Pose priors (opt-in; none by default).  The LM then minimises
 *     C(x) = sum_voxels lambda_min + sum_k 1/2 |L_k r_k(x)|^2
 * with H, g the exact gradient and the Gauss-Newton Hessian of C; the averaged costs (is_avg, the trace's residual1/2,
 * cost_avg) divide the whole sum by the voxel count.  With A = T_i O_i, B = T_j O_j (O = body-frame offset, R row-major | t like a
 * pose; twelve zeros mean identity) and the residual order [rotation; position] of the tangent:
 *   LVBA_PRIOR_POSE      r = [Log(Rm^T R_A); p_A - pm]                       meas = (Rm | pm)
 *   LVBA_PRIOR_POSITION  r = p_A - z, 3 rows, top-left 3 x 3 of sqrt_info    meas[9..11] = z (meas[0..8] not read); p_O = lever arm
 *   LVBA_PRIOR_RELATIVE  r = [Log(Rm^T R_A^T R_B); R_A^T (p_B - p_A) - pm]   meas = T_ij measured, i != j
 * sqrt_info is the 6 x 6 square-root information matrix L, row-major.  Indices are caller pose indices.
 *   lvba_balm_set_priors       n = 0 clears.  Before the first cost / eval / solve / refine call any pairs may be joined (a
 *                              relative prior is an edge of the pose graph: ordering, band and dissection take it in); after it the
 *                              priors may only be replaced if every relative pair is already a block of the store, else
 *                              LVBA_ERR_STATE.  LVBA_ERR_ARG: unknown kind, index out of range, i == j for RELATIVE, a non-finite
 *                              value, a measurement / offset rotation that is not orthonormal within 1e-6.  A refused call leaves
 *                              the handle as it was.  A grouped handle (lvba_balm_set_groups) refuses priors (LVBA_ERR_STATE).
 *                              Sharded handles: a collective call like cost / eval / refine -- every rank makes it, with the
 *                              same priors; the next collective call checks that (one small all-reduce, also made once at the
 *                              set-up of every sharded handle) and returns LVBA_ERR_ARG on every rank if they differ.
 *                              At most 2^22 priors.
 *   lvba_balm_prior_residuals  e [n][6] the whitened residuals L r (POSITION: e[k][0..2], e[k][3..5] = 0), cost = sum 1/2 |e|^2;
 *                              either may be NULL. */
#define LVBA_PRIOR_POSE 0
#define LVBA_PRIOR_POSITION 1
#define LVBA_PRIOR_RELATIVE 2
typedef struct {
    int32_t kind, i, j, reserved;
    double meas[12];
    double offset_i[12], offset_j[12];
    double sqrt_info[36];
} lvba_prior;
int32_t lvba_balm_set_priors(lvba_balm_t h, int32_t n, const lvba_prior *priors);
int32_t lvba_balm_prior_residuals(lvba_balm_t h, const double *poses, double *e, double *cost);

/* Marginal pose covariance (opt-in).
 *   C(x) = sum_voxels lambda_min + sum_k 1/2 |L_k r_k(x)|^2 is the cost the LM minimises (the priors above).  H(x) is its Hessian
 *   exactly as lvba_balm_eval forms it: the exact second-order voxel part plus the Gauss-Newton prior part, undamped (u = 0), not
 *   averaged.
 *   The covariance returned is Sigma = H(x)^-1 in the tangent of BALM's retraction (R <- R Exp(dphi), p <- p + dp, order
 *   [dphi; dp], bavoxel.hpp:723-727), in the caller's pose order.
 *   The gauge is fixed in one of two ways:
 *     anchor >= 0  that caller pose is held fixed: its rows and columns are removed, which is equivalent to replacing them by the
 *                  identity and zero couplings before factorising.  The anchor's own block (and its pair blocks) are returned
 *                  as zeros.
 *     anchor = -1  H itself must be positive definite, for example because priors fix the frame.
 *   The result is the inverse Hessian of C in C's units.  Turning it into a metric covariance needs a noise model: lambda_min is a
 *   mean squared point-to-plane distance per voxel, not a whitened residual, so Sigma is not a covariance in metres / radians
 *   until the caller scales it by the noise variance it believes in.
 * diag [n_poses][36] row-major (may be NULL); for each requested pair k (i != j, caller indices) blocks[k][6r+c] =
 * Cov(delta_i[r], delta_j[c]) and avail[k] = 1 if the pair lies in the handle's band (every pair that shares a voxel or a relative
 * prior does), else avail[k] = 0 and the block is NaN.  Collective on sharded handles (every rank makes the call; results are
 * bitwise equal on all ranks).
 *   LVBA_NUM_FACTORIZATION  a pivot d_i <= min_pivot_ratio * A_ii or non-finite: H is not positive definite at these poses (free
 *                           gauge, or not at a minimum).  Nothing is written to the outputs.
 *   LVBA_ERR_ARG            anchor or a pair index out of range, or i == j.
 *   LVBA_ERR_STATE          between lvba_balm_lm_begin and lvba_balm_lm_end.
 *   LVBA_ERR_UNSUPPORTED    grouped (lvba_balm_set_groups) or dissected (nd_kind != 0) handles.
 * Like lvba_balm_eval the call replaces the handle's last evaluation; a later lvba_balm_solve needs a fresh lvba_balm_eval.
 * Nothing else changes: a refinement after a covariance call gives bitwise the poses it gives without one. */
typedef struct {
    int32_t anchor;            /* caller pose held fixed, or -1: H must be positive definite (priors fix the frame) */
    int32_t reserved;
    double  min_pivot_ratio;   /* refuse if a pivot d_i <= min_pivot_ratio * A_ii or is non-finite; default 1e-10 */
} lvba_cov_opts;
void lvba_cov_default_opts(lvba_cov_opts *o);
int32_t lvba_balm_covariance(lvba_balm_t h, const double *poses, const lvba_cov_opts *opts,
                             double *diag, int64_t n_pairs, const int32_t *pi, const int32_t *pj,
                             double *blocks, uint8_t *avail);

/* Robust loss on the voxel costs (opt-in; none by default).  With a loss rho of kind LVBA_LOSS_* and scale a in metres (the kinds and
 * formulas of lvba_visual_set_loss below, b = a^2) and s_v = lambda_min(v), a mean squared point-to-plane distance in m^2:
 *     C(x) = sum_v rho(s_v) + sum_k 1/2 |L_k r_k(x)|^2        the priors are never under the loss
 *     g    = sum_v rho'(s_v) g_v                              the exact gradient of C
 *     H    = sum_v rho'(s_v) H_v                              H_v: the exact second-order voxel Hessian
 * A voxel is down-weighted when its RMS plane distance exceeds a: exactly so for HUBER and TUKEY, as the knee of SOFTLONE and
 * CAUCHY.  Not for ARCTAN: that kind (as Ceres defines it) weighs with 1 / (1 + s^2 / a^2), comparing s with a rather than with
 * a^2, so with s in m^2 and a in m only voxels with lambda_min near a lose weight -- at a ~ 0.1 m hardly any.
 * There is no factor 1/2 on the voxel sum: TRIVIAL is exactly the cost without a loss.  The term rho''(s_v) g_v g_v^T is left out of H on purpose: every kind has rho'' <= 0, so the term is negative
 * semidefinite and the kept matrix majorises the true Hessian -- the choice the visual stage makes (Ceres' corrector takes only its
 * scaling branch for rho'' <= 0); keeping it would need a fourth column in every per-factor record of the Hessian assembly.
 * lvba_balm_covariance returns the inverse of this H.  The LM loop is damping_iter unchanged on the robust quantities: residual1/2,
 * the averaged costs, q, q1 and the exit test all use C.
 *   lvba_balm_set_loss         NULL or TRIVIAL restores the default.  LVBA_ERR_ARG (handle unchanged): unknown kind, or a non-trivial
 *                              kind with a scale that is not finite and > 0.  LVBA_ERR_STATE: between lvba_balm_lm_begin and
 *                              lvba_balm_lm_end; allowed at any other time, on plain, grouped and dissected handles, with priors.
 *                              Like lvba_balm_eval it replaces the handle's last evaluation (a later lvba_balm_solve needs a fresh
 *                              one).  Sharded handles: a collective call like lvba_balm_set_priors -- every rank makes it, with the same
 *                              loss; the next collective call checks that and returns LVBA_ERR_ARG on every rank if they differ.
 *   lvba_balm_voxel_residuals  lambda_min [n_voxels] and weight [n_voxels] = rho'(lambda_min) at `poses`, in the CALLER's voxel order
 *                              (whatever order the handle keeps its voxels in); either may be NULL.  Without a loss every weight is 1.
 *                              Rank-local on a sharded handle (its own voxels) -- but the handle's set-up is collective: make
 *                              the first cost / eval / refine call (on every rank) before this one.
 * lvba_version() is unchanged by these calls (112); a client detects them by looking the symbols up.
 * A TUKEY loss can leave a pose whose voxels all have weight zero: a rank-deficient problem, reported as any other
 * (LVBA_NUM_FACTORIZATION from the solve / the LM row); there is no fallback. */
#define LVBA_LOSS_TRIVIAL 0
#define LVBA_LOSS_HUBER 1
#define LVBA_LOSS_SOFTLONE 2
#define LVBA_LOSS_CAUCHY 3
#define LVBA_LOSS_ARCTAN 4
#define LVBA_LOSS_TUKEY 5
typedef struct {
    int32_t kind;         /* LVBA_LOSS_* */
    int32_t reserved;
    double scale;         /* a > 0, finite; ignored for TRIVIAL */
} lvba_loss;
int32_t lvba_balm_set_loss(lvba_balm_t h, const lvba_loss *loss);
int32_t lvba_balm_voxel_residuals(lvba_balm_t h, const double *poses, double *lambda_min, double *weight);

/* Profiling (HIP events around the stages, on the stream the kernels are launched on). */
int32_t lvba_balm_set_profiling(lvba_balm_t h, int32_t enable);
int32_t lvba_balm_get_profile(lvba_balm_t h, lvba_prof_t *out, int32_t reset);

/* Pose ordering used internally: perm[internal] = caller pose index (n_poses entries). */
int32_t lvba_balm_get_ordering(lvba_balm_t h, int32_t *perm);

/* What the damped solve would look like on n_ranks ranks: the nested-dissection plan csrc/nd_plan.h makes of this problem's
 * co-visibility graph (arcs dealt out over the ranks, separator system) and its cost model in ms per solve, next to the band
 * factorisation's (two ranks at best).  A MODEL, in the solver's own measured units (launches on the serial chain x us per
 * launch, flops / sustained rate); nd_ms = 0: no partition exists.  Needs >= 256 poses. */
typedef struct {
    int32_t n_ranks, arcs, sep_poses, sep_band_blocks, max_arc_poses, max_arc_band_blocks;
    double band_ms, nd_ms;
} lvba_nd_model_t;
int32_t lvba_balm_nd_model(lvba_balm_t h, int32_t n_ranks, lvba_nd_model_t *out);

/* Multi-GPU (one process per GPU): factors are sharded by voxel range across ranks; every eval
 * all-reduces {block-band H, g, cost} and every cost pass all-reduces one double, over RCCL.
 * uid is an ncclUniqueId (128 bytes) created on rank 0 and distributed by the caller. */
int32_t lvba_dist_unique_id(char uid[128]);
int32_t lvba_balm_dist_init(lvba_balm_t h, int32_t n_ranks, int32_t rank, const char uid[128]);
/* The same with the CALLER'S transport instead of RCCL (an MPI job that already owns a communicator; a test harness that runs
 * several ranks as host threads on one device, where RCCL refuses a duplicate GPU -- tests/host_transport.cpp).  `fn` must
 * all-reduce `count` elements of type `dtype` of the DEVICE buffer `device_buf` in place over the n_ranks ranks with `op`,
 * ordered after the work already enqueued on `hip_stream` (a hipStream_t) and visible to work enqueued on it afterwards;
 * every rank must obtain bitwise the same result (sum in a fixed rank order), as RCCL guarantees for its own.  It returns 0
 * on success.  The library calls it from the thread that calls the library, never concurrently for one handle. */
#define LVBA_DT_F64 0
#define LVBA_DT_I64 1
#define LVBA_DT_I32 2
#define LVBA_DT_U8 3
#define LVBA_OP_SUM 0
#define LVBA_OP_MAX 1
typedef int32_t (*lvba_allreduce_fn)(void *ctx, void *device_buf, size_t count, int32_t dtype, int32_t op, void *hip_stream);
int32_t lvba_balm_dist_init_external(lvba_balm_t h, int32_t n_ranks, int32_t rank, lvba_allreduce_fn fn, void *ctx);

/* ===================================================================================================
 * Visual stage: replaces the ceres::Problem ... ceres::Solve region of LvbaSystem::optimizeCameraPoses
 * (src/lvba_system.cpp:1571-1665) with the cost functors of include/utils.hpp:51-147.
 *   camera   = T_cam<-world: q [w,x,y,z] (memory order of src/lvba_system.cpp:1516) + t; camera 0 is held
 *              constant (:1582-1583); quaternions move on ceres::EigenQuaternionManifold applied to that memory
 *              as the reference does (:1579) -- see DESIGN.md
 *   landmark = X_w [3]; a landmark whose `valid` flag is 0 (no plane found, :1598-1603) is dropped together with
 *              its reprojection observations and is returned unchanged
 *   residuals: per observation the whitened Brown-Conrady reprojection error (2), per landmark the whitened
 *              point-to-plane distance sqrt(s^2+1e-12)/sigma (1); by default no loss function (:1630,1639), each
 *              family may take a robust loss (lvba_visual_set_loss).  cost = 1/2 sum rho(s), s = |r|^2 of a block
 *   solver:    Levenberg-Marquardt trust region with Ceres 2.1 defaults restated (Jacobi scaling, LM diagonal
 *              clamp(diag)/radius, radius schedule, tolerances), landmark blocks eliminated (Schur), reduced
 *              camera system solved by the same LDL^T as the LiDAR stage.
 * =================================================================================================== */
typedef struct lvba_visual_s *lvba_visual_t;

typedef struct {
    int32_t max_iter;               /* 50     src/lvba_system.cpp:1573 */
    int32_t reserved;
    double initial_radius;          /* 1e4    Ceres default initial_trust_region_radius */
    double max_radius;              /* 1e16 */
    double min_radius;              /* 1e-32 */
    double min_relative_decrease;   /* 1e-3 */
    double min_lm_diagonal;         /* 1e-6 */
    double max_lm_diagonal;         /* 1e32 */
    double function_tolerance;      /* 1e-6 */
    double gradient_tolerance;      /* 1e-10 */
    double parameter_tolerance;     /* 1e-8 */
} lvba_visual_opts;

#define LVBA_TERM_NO_CONVERGENCE 0  /* max_iter reached */
#define LVBA_TERM_FUNCTION 1
#define LVBA_TERM_PARAMETER 2
#define LVBA_TERM_GRADIENT 3
#define LVBA_TERM_RADIUS 4
#define LVBA_TERM_FAILURE 5         /* linear solver failed repeatedly / non-finite cost */

/* one row per iteration, iteration 0 = the initial evaluation (like Ceres' progress table) */
typedef struct {
    int32_t iter;
    int32_t accepted;     /* step successful (always 1 for iteration 0) */
    int32_t valid;        /* linear solve produced a finite step with positive model decrease */
    int32_t reserved;
    double cost;          /* 1/2 sum rho(s): the new cost if accepted, the rejected candidate's cost otherwise */
    double cost_change;
    double step_norm;
    double radius;        /* trust-region radius after this iteration's update */
    double rho;           /* relative decrease (step quality) */
    double gradient_max_norm;
} lvba_visual_trace;

void lvba_visual_default_opts(lvba_visual_opts *opts);

/* obs_off [n_tracks+1] CSR offsets of each landmark's (de-duplicated, inlier) observations; obs_cam [O] in
 * [0,n_cams); obs_uv [O][2] pixels; plane [n_tracks][4] = (n, d); valid [n_tracks]; intr = fx fy cx cy k1 k2 p1 p2
 * (already scaled, src/dataset_io.cpp:59-62); sigma_px = 0.5, sigma_plane = 0.01 upstream (:1590-1591). */
int32_t lvba_visual_create(int32_t n_cams, int64_t n_tracks, const int64_t *obs_off, const int32_t *obs_cam,
                           const double *obs_uv, const double *plane, const uint8_t *valid, const double intr[8],
                           double sigma_px, double sigma_plane, int32_t device, lvba_visual_t *out);
int32_t lvba_visual_destroy(lvba_visual_t h);

/* Sizes of the packed problem in the fields of lvba_balm_info_t that apply: n_poses = cameras, n_voxels = landmarks with a
 * plane (the active ones), n_factors = their observations, n_pairs, n_blocks (off-diagonal camera blocks of the reduced
 * system), band_blocks, use_band, hess_bytes, device_bytes. */
int32_t lvba_visual_info(lvba_visual_t h, lvba_balm_info_t *info);
/* The pair-pass layout of the reduced camera system (as lvba_balm_pair_layout: items are runs of camera pairs of one block). */
int32_t lvba_visual_pair_layout(lvba_visual_t h, lvba_pair_layout_t *out, int64_t *item_len, int64_t *item_slot, int64_t cap);
/* The launch layout of the kernels that form the reduced camera system and back-substitute (as lvba_balm_eval_layout). */
int32_t lvba_visual_eval_layout(lvba_visual_t h, lvba_eval_layout_t *out);

/* Multi-GPU: landmark tracks are sharded over the ranks (any partition; contiguous ranges as for the voxels), the cameras are
 * replicated.  Every rank creates its handle from ITS tracks (X, plane, valid and the observation arrays of that shard) and
 * calls this before the first cost / linearize / refine call.  Per LM iteration the ranks all-reduce the reduced camera system
 * [S | rhs] (only the blocks of the union pattern), 12 M per-camera sums (the LM diagonal and the gradient test need the
 * whole diag(Jc^T Jc), Jc^T r) and five scalars; the reduced system is solved on every rank.  All ranks return bitwise the same
 * cameras and trace; X holds the rank's own landmarks.  uid as for lvba_balm_dist_init. */
int32_t lvba_visual_dist_init(lvba_visual_t h, int32_t n_ranks, int32_t rank, const char uid[128]);
int32_t lvba_visual_dist_init_external(lvba_visual_t h, int32_t n_ranks, int32_t rank, lvba_allreduce_fn fn, void *ctx);

/* 1/2 sum rho(s) over the residual blocks of the active landmarks at (q [M][4], t [M][3], X [n_tracks][3]). */
int32_t lvba_visual_cost(lvba_visual_t h, const double *q, const double *t, const double *X, double *cost);

/* Linearise at the given point with trust-region radius `radius` (Jacobi scaling taken from THIS Jacobian, as at
 * Ceres' iteration 0): the reduced camera system S [6M x 6M] (symmetric; camera 0's block is decoupled) and its
 * right-hand side rhs [6M] in the scaled tangent variables, caller camera order.  For tests / inspection. */
int32_t lvba_visual_linearize(lvba_visual_t h, const double *q, const double *t, const double *X, double radius,
                              double *S, double *rhs, double *cost);

/* Solve the reduced camera system the last lvba_visual_linearize left on this handle, with the kernels a refinement would use:
 * x [6M] = -S^-1 rhs in the scaled tangent variables, caller camera order (camera 0: zeros).  *solver (may be NULL) tells
 * which kernels ran: 0 = LDL^T, 1 = block cyclic reduction with block rows of 32 scalars, 2 = with block rows of 64.
 * LVBA_NUM_FACTORIZATION on a pivot <= 0; LVBA_ERR_STATE without a prior lvba_visual_linearize on the handle (an
 * lvba_visual_refine in between replaces the system) and on a sharded handle.  For tests / inspection. */
int32_t lvba_visual_solve(lvba_visual_t h, double *x, int32_t *solver);

/* Robust losses, Ceres 2.1 semantics (loss_function.cc, corrector.cc): a residual block with squared norm s = |f|^2
 * contributes 1/2 rho(s) to the cost, and its residual and Jacobian enter the linearisation as sqrt(rho'(s)) f,
 * sqrt(rho'(s)) J (every kind here has rho'' <= 0).  `scale` = a, in whitened residual units:
 *   TRIVIAL   rho = s (default: the reference's nullptr)
 *   HUBER     s <= a^2: s, else 2 a sqrt(s) - a^2         SOFTLONE  2 a^2 (sqrt(1 + s/a^2) - 1)
 *   CAUCHY    a^2 log(1 + s/a^2)                          ARCTAN    a atan2(s, a)
 *   TUKEY     s <= a^2: a^2/3 (1 - (1 - s/a^2)^3), else a^2/3
 * The reference's own (unused) constants, :1585-1586: HUBER 1.0 on the reprojection blocks (0.5 px at sigma_px 0.5), HUBER 0.1
 * on the plane blocks (1 mm at sigma_plane 0.01). */
/* (LVBA_LOSS_* and lvba_loss are defined above, with lvba_balm_set_loss: both stages share them) */

/* Loss of the reprojection blocks (one 2-vector per observation) and of the plane blocks (one per active landmark); NULL =
 * TRIVIAL.  Kept on the handle for every later cost / linearize / refine call.  An unknown kind, or a non-trivial kind with a
 * scale that is not finite and > 0, returns LVBA_ERR_ARG and leaves the handle unchanged.  Sharded handles: every rank must set
 * the same losses; each cost / linearize / refine call checks this with one small all-reduce and fails with LVBA_ERR_ARG on
 * every rank otherwise. */
int32_t lvba_visual_set_loss(lvba_visual_t h, const lvba_loss *reproj, const lvba_loss *plane);

/* Camera pose priors (opt-in; none by default).  The refinement then minimises
 *     cost = 1/2 sum_blocks rho(s)  +  1/2 sum_k |L_k r_k|^2            the priors are never under a loss
 * The pose a prior sees is the camera's pose in the world, T_k = T_world<-cam_k = (R(q_k)^T, -R(q_k)^T t_k) (q normalised as
 * everywhere in this stage); with A = T_i O_i, B = T_j O_j the three kinds, the residual order [rotation; position], the
 * offsets (twelve zeros = identity; p_O of a POSITION prior = lever arm) and the 6 x 6 row-major sqrt_info are exactly those of
 * lvba_balm_set_priors above -- lvba_prior is reused as it is, i / j are caller camera indices.  An offset O = T_cam<-imu states
 * a prior on the body pose T_world<-imu directly.  Each prior is one more residual block with a trivial loss on the cameras
 * (i[, j]): its whitened Jacobian in the visual tangent (EigenQuaternionManifold on the [w,x,y,z] memory, t additive) counts in
 * the Jacobi scaling, the LM diagonal, the gradient max, the reduced camera system, the model cost change and every cost of the
 * trace.  Camera 0 stays constant: a prior on it contributes its cost only, a RELATIVE prior with it the other camera's side.
 *   lvba_visual_set_priors       n = 0 clears.  Before the first cost / linearize / refine / prior_residuals call any pairs may be joined (a
 *                                relative prior is an edge of the camera graph: ordering, band and solver choice take it in); after
 *                                it the priors may only be replaced if every relative pair is already a block of the store, else
 *                                LVBA_ERR_STATE.  LVBA_ERR_ARG for an unknown kind, an index out of [0, n_cams), i == j for
 *                                RELATIVE, a non-finite value, a measurement / offset rotation that is not orthonormal within
 *                                1e-6: the handle as it was.  Sharded handles: every rank sets the same priors (the cameras are
 *                                replicated, rank 0 adds them); each cost / linearize / refine call checks this together with the
 *                                losses and fails with LVBA_ERR_ARG on every rank otherwise.  At most 2^22 priors.
 *   lvba_visual_prior_residuals  e [n][6] the whitened residuals L r (POSITION: e[k][0..2], e[k][3..5] = 0), cost = sum 1/2 |e|^2;
 *                                either may be NULL.  Rank-local on a sharded handle (call it after the first cost / linearize /
 *                                refine call there).  Like those calls it lays out the store on its first use: relative priors
 *                                that join new pairs of cameras go in before it as well.
 * A handle without priors launches no kernel of this part and returns bitwise what it returned before they existed.
 * lvba_visual_residual_sq is unchanged. */
int32_t lvba_visual_set_priors(lvba_visual_t h, int32_t n, const lvba_prior *priors);
int32_t lvba_visual_prior_residuals(lvba_visual_t h, const double *q, const double *t, double *e, double *cost);

/* Whitened squared norms s of the residual blocks at (q, t, X), before any loss: obs_sq [O] per caller observation
 * (O = obs_off[n_tracks] - obs_off[0], caller order), plane_sq [n_tracks] per landmark; NaN for landmarks with valid == 0 and
 * their observations.  Which blocks a loss down-weights: s > a^2.  Rank-local on a sharded handle (its own tracks; call it
 * after the first cost / linearize / refine call there). */
int32_t lvba_visual_residual_sq(lvba_visual_t h, const double *q, const double *t, const double *X, double *obs_sq,
                                double *plane_sq);

/* The solve: refines q, t, X in place (quaternions re-normalised on write-back, :1651-1657). */
int32_t lvba_visual_refine(lvba_visual_t h, double *q, double *t, double *X, const lvba_visual_opts *opts,
                           lvba_visual_trace *trace, int32_t trace_cap, int32_t *n_trace, int32_t *termination);

/* ---- voxel front-end: raw scans -> the packed LiDAR-BA problem, on the device ---------------------------------------
 * Replaces the construction that precedes every damping_iter call (src/lvba_system.cpp:247-258, :365-377, :1498-1506):
 *   lvba_voxmap_build       <- cut_voxel (include/BALM/bavoxel.hpp:799-836) for every frame, then, for every root,
 *                              OCTO_TREE_NODE::recut (:391-464, judge_eigen :335-352)
 *   lvba_voxmap_to_balm     <- OCTO_TREE_NODE::tras_opt (:466-474) into VOX_HESS::push_voxel (:45-54)
 *   lvba_voxmap_find_planes <- recompute_local_planes (src/lvba_system.cpp:1531-1565) +
 *                              OCTO_TREE_NODE::findCorrespondPoint (bavoxel.hpp:320-333)
 * Kept from the reference: fp32 points promoted to double; root key = C truncation of a FLOAT quotient that had 1
 * subtracted when negative; float voxel centres / quarter lengths; octant test `double > float`; a node with fewer
 * than min_points points is dropped, one whose lambda_min/lambda_max exceeds eigen_ratio[layer] is split (dropped at
 * layer 2); PointCluster sums accumulate in cloud order (results are bit-identical to PointCluster::push).
 * Voxels come out sorted by (root key x,y,z, octant path); the reference's unordered_map order is unspecified. */
typedef struct lvba_voxmap_s *lvba_voxmap_t;
typedef struct {
    double voxel_size;      /* root voxel edge (stage1_root_voxel_size_ / stage2_root_voxel_size_) */
    float eigen_ratio[4];   /* eigen_ratio_array (bavoxel.hpp:17, include/dataset_io.h:77,80); [3] unused as upstream */
    int32_t min_points;     /* min_ps = 15 (bavoxel.hpp:24) */
    int32_t layer_limit;    /* must be 2 (bavoxel.hpp:13) */
} lvba_voxel_opts;
typedef struct {
    int64_t n_points, n_roots, n_planes; /* points hashed; root voxels; PLANE nodes (admitted or not) */
    int64_t n_voxels, n_factors;         /* admitted voxels (>= 2 observing frames) and their cluster slots */
    /* host wall clock of the build phases, ms (each ends on a stream synchronise): host->device copy of the clouds
     * (lvba_voxmap_build only), key kernel, root sort + gather + root table, octree walk (count), octree walk (write) */
    double upload_ms, key_ms, sort_ms, count_ms, write_ms;
} lvba_voxmap_info_t;
void lvba_voxel_default_opts(lvba_voxel_opts *opts);

/* frame_points[f] -> host memory of frame f's cloud: frame_count[f] points, x,y,z as the first three floats of every
 * point_stride_bytes (12 for packed xyz, sizeof(pcl::PointXYZINormal) = 48 for the reference's PointType);
 * poses [n_frames][12].  Fails with LVBA_ERR_ARG on a non-finite point. */
int32_t lvba_voxmap_build(int32_t device, int32_t n_frames, const void *const *frame_points,
                          const int64_t *frame_count, int32_t point_stride_bytes, const double *poses,
                          const lvba_voxel_opts *opts, lvba_voxmap_t *out);
int32_t lvba_voxmap_destroy(lvba_voxmap_t h);

/* The same, in two steps, for callers that voxelise the same clouds more than once (the reference re-cuts the anchor
 * clouds for stage 1, stage 2 and the visual stage, src/lvba_system.cpp:365-377,1498-1506, and the raw scans window by
 * window, :232-258): lvba_scans_create copies the clouds to the device once; lvba_voxmap_build_scans builds the map of
 * frames [frame_begin, frame_begin + n_frames) at poses [n_frames][12] (pose / frame indices in the outputs are
 * relative to frame_begin, as cut_voxel's fnum is relative to the window). */
typedef struct lvba_scans_s *lvba_scans_t;
int32_t lvba_scans_create(int32_t device, int32_t n_frames, const void *const *frame_points,
                          const int64_t *frame_count, int32_t point_stride_bytes, lvba_scans_t *out);
int32_t lvba_scans_destroy(lvba_scans_t scans);
int32_t lvba_voxmap_build_scans(lvba_scans_t scans, int32_t frame_begin, int32_t n_frames, const double *poses,
                                const lvba_voxel_opts *opts, lvba_voxmap_t *out);

int32_t lvba_voxmap_info(lvba_voxmap_t h, lvba_voxmap_info_t *info);
/* The front-end keeps its device workspaces in a per-process cache between maps (hipMalloc/hipFree of 100 MB-class
 * buffers would otherwise dominate small maps); this returns the cached bytes to the driver.  Returns bytes freed. */
int64_t lvba_release_cached_memory(void);
/* Host copies of the admitted voxels in lvba_balm_create's layout (any pointer may be NULL): voxel_off [V+1],
 * pose_idx [F], clusters [F][10], voxel_key [V][4] = root key x, y, z and layer | o1 << 4 | o2 << 8. */
int32_t lvba_voxmap_export(lvba_voxmap_t h, int64_t *voxel_off, int32_t *pose_idx, double *clusters,
                           int64_t *voxel_key);
/* The VOX_HESS of this map (poses = the n_frames of the build), ready for lvba_balm_refine. */
int32_t lvba_voxmap_to_balm(lvba_voxmap_t h, lvba_balm_t *out);
/* plane [n][4] = (unit normal, d = -n.centre) and valid [n] for n world points X [n][3]; invalid -> zeros. */
int32_t lvba_voxmap_find_planes(lvba_voxmap_t h, int64_t n, const double *X, double *plane, uint8_t *valid);

/* ---- track -> landmark initialisation (the step before the visual solve) ------------------------------------------------
 *   lvba_triangulate_tracks <- TriangulateTrackDLT (src/lvba_system.cpp:50-111) + ComputeMeanReproj (:8-48) for every track:
 *   DLT on the undistorted normalised pixels (undistortPixelToNormalized, include/utils.hpp:207-233: 8 fixed-point
 *   iterations of the Brown-Conrady model), smallest eigenvector of the 4x4 A^T A, X = Xh.xyz / Xh.w, then the mean pixel
 *   error of X over the track.  Tracks are CSR (obs_off [n+1] from 0, obs_cam [O], obs_uv [O][2]), one observation per
 *   image as the reference's selected_ids holds them; Rcw [M][9] row-major and tcw [M][3] are T_cam<-world.
 *   ok[i] = 1 iff the track has >= 4 observations, >= 8 DLT rows, |Xh.w| >= 1e-12, finite X and >= 4 valid reprojections
 *   (mean_reproj = +inf otherwise; the caller applies its own reproj_mean_thr_px_ as at :1143-1146).
 *   LVBA_ERR_ARG, before any device work and with the outputs untouched: obs_off does not start at 0 or decreases somewhere
 *   (the kernel would walk observations past obs_off[n_tracks]). */
int32_t lvba_triangulate_tracks(int32_t device, int32_t n_cams, int64_t n_tracks, const int64_t *obs_off,
                                const int32_t *obs_cam, const double *obs_uv, const double *Rcw, const double *tcw,
                                const double intr[8], double *X, double *mean_reproj, int32_t *count, uint8_t *ok);

/* ---- LiDAR-assisted landmark initialisation: depth images + per-track fusion ---------------------------------------------
 *   lvba_depth_render <- LvbaSystem::buildGridMapFromOptimized (src/lvba_system.cpp:1266-1338) + generateDepthWithVoxel
 *   (:835-919): every scan point in the world frame (scan_poses [n_frames][12], T_world<-body of the REFINED trajectory) is
 *   hashed into voxel_size (reference: 0.5 m) voxels; image m sees the voxels touched by the scans with
 *   |scan_time - image_time| <= half_window_s (reference: 0.5 s; scan_times ascending; the reference passes the image id
 *   through std::to_string, i.e. rounds it to 1e-6 s -- the caller does that) and ALL map points of those voxels are
 *   z-buffered through camera m (Rcw [n][9], tcw [n][3], intr = fx fy cx cy k1 k2 p1 p2): pixel (int)u, (int)v, Z < 1e-3
 *   skipped, smallest (float)Z wins, 0 = no return.  Images stay on the device.
 *   lvba_depth_upload makes a handle from host images [n][height][width] (depth from another source).
 *   lvba_fuse_tracks <- the per-component part of LvbaSystem::BuildTracksAndFuse3D (:1000-1225): tracks are the BFS
 *   components in CSR form (obs_off [n+1] from 0, obs_img [O], obs_uv [O][2] float keypoint coordinates, observations in BFS
 *   order, several per image allowed).  Per track: the depth-fused candidate (fetchDepthBilinear, back-projection through the
 *   distortion model, 0.12 m consistency with the first valid observation, first observation per image, greedy view-angle
 *   filter, mean reprojection error), the triangulation candidate (DLT over the first observation of every image, the same
 *   filter around the seed, DLT again over >= 4 kept observations), then the reference's selection.  depth may be NULL
 *   (triangulation candidate only).  status[t] = 0 dropped / 1 triangulated / 2 depth-fused; X [n][3]; mean_reproj [n]
 *   (+inf when dropped); kept [O] = the track's inlier_indices as a mask.  Where the reference iterates a
 *   std::unordered_map<int,int> of images (unique_id :994, best_id :1051, kept_id_depth :1064), images are visited in the order libstdc++ gives that
 *   container for the reference's reserve() and insertion sequence (bucket = key mod the rehash policy's prime, a new node
 *   goes to the front of its bucket and a new bucket to the front of the list: csrc/tracks_device.h umap_order), because
 *   the greedy view-angle filter's survivors depend on it.
 *   An observation whose pixel is NaN or +-inf has no depth point (the reference's fetchDepthBilinear would index with it,
 *   which is undefined; csrc/fusion_device.h depth_world_point) and, having no undistorted point, adds no DLT rows; it still
 *   counts as the observation of its image.
 *   LVBA_ERR_ARG, before any device work and with the outputs untouched: obs_off does not start at 0 or decreases somewhere;
 *   obser_thr < 1; min_view_angle_deg NaN or outside [0, 180]; reproj_mean_thr_px NaN or negative.  Image ids outside
 *   [0, n_images) are no error: such observations are skipped. */
typedef struct lvba_depth_s *lvba_depth_t;
int32_t lvba_depth_render(lvba_scans_t scans, const double *scan_poses, const double *scan_times, int32_t n_images,
                          const double *image_times, const double *Rcw, const double *tcw, const double intr[8],
                          int32_t width, int32_t height, double half_window_s, double voxel_size, lvba_depth_t *out);
int32_t lvba_depth_upload(int32_t device, int32_t n_images, int32_t width, int32_t height, const float *depth,
                          lvba_depth_t *out);
int32_t lvba_depth_info(lvba_depth_t depth, int32_t *n_images, int32_t *width, int32_t *height);
int32_t lvba_depth_download(lvba_depth_t depth, int32_t image, float *out);
void lvba_depth_destroy(lvba_depth_t depth);

typedef struct lvba_fuse_opts {
    int32_t obser_thr;          /* minimum observations / images per track (config obser_thr, default 3) */
    int32_t reserved;
    double min_view_angle_deg;  /* greedy view-angle filter (config min_view_angle_deg, default 8) */
    double reproj_mean_thr_px;  /* acceptance threshold of a candidate's mean reprojection error (default 3) */
} lvba_fuse_opts;
void lvba_fuse_default_opts(lvba_fuse_opts *opts);
int32_t lvba_fuse_tracks(int32_t device, lvba_depth_t depth, int32_t n_images, const double *Rcw, const double *tcw,
                         const double intr[8], int64_t n_tracks, const int64_t *obs_off, const int32_t *obs_img,
                         const float *obs_uv, const lvba_fuse_opts *opts, uint8_t *status, double *X, double *mean_reproj,
                         uint8_t *kept);

/* ---- window BA: raw scans + odometry -> anchor frames --------------------------------------------------------------
 *   lvba_window_ba <- LvbaSystem::runWindowBA  src/lvba_system.cpp:204-310 : for every window of window_size frames the voxel
 *   map at the odometry poses (:247-257), the "fewer than 3 plane voxels per frame -> skip" rule (:258-262), damping_iter
 *   (:264), re-alignment of the optimised window to its first odometry pose (:268-279), relative poses to the anchor and the
 *   merged cloud in the anchor frame with fp32 write-back (:284-299, pl_transform include/BALM/tools.hpp:385-395) and
 *   down_sampling_voxel2 (tools.hpp:300-359; survivors come out sorted by voxel key, upstream order is unspecified).
 * Outputs follow the reference's members: rel_poses [n][12] = rel_poses_to_anchor_ (identity for frames of skipped windows),
 * anchor_index [n] = anchor_index_per_frame_ (-1 when skipped), anchor_poses [<= ceil(n/w)][12] = odometry pose of each
 * window's first frame, anchor_scans = the merged, down-sampled clouds as a device-resident scan set (destroy with
 * lvba_scans_destroy), window_poses [n][12] (may be NULL) = the optimised poses before re-alignment, win_info
 * [ceil(n/w)] (may be NULL). */
typedef struct {
    int32_t window_size;    /* window_ba_size_ (10; config.yaml 20) */
    int32_t use_rel;        /* use_window_ba_rel_ */
    double anchor_leaf;     /* anchor_leaf_size_ (0.1; config.yaml 0.01); < 0.001 disables the down-sampling */
    lvba_voxel_opts voxel;  /* stage1_root_voxel_size_ and the eigen_ratio_array in effect (bavoxel.hpp:17 until a stage sets it) */
    lvba_balm_opts lm;
    int32_t merge_only;     /* 1: no map, no LM, no skip rule -- every window is merged at the given poses (rel = anchor^-1 o pose) and
                               down-sampled: the anchor clouds optimizeCameraPoses rebuilds from the refined poses (:1464-1487) */
    int32_t lm_mode;        /* 0: the damping_iter of all windows in lock-step as one grouped problem (lvba_balm_refine_groups;
                               default), 1: one window at a time.  The windows are independent either way; results agree to
                               rounding */
} lvba_window_opts;
typedef struct {
    int32_t start, n_frames, skipped, anchor; /* anchor = index into anchor_poses / anchor_scans, -1 if skipped */
    int32_t n_iter, lm_status;
    int64_t n_voxels, n_factors, n_anchor_points;
    double cost_first, cost_last;             /* averaged LiDAR cost before / after the window's damping_iter */
    double map_ms, solve_ms, merge_ms;        /* host wall clock: voxel map, problem set-up + LM (lm_mode 0: the joint problem's
                                                 time shared out evenly over its windows), anchor merge + down-sampling */
    double setup_ms;                          /* the part of solve_ms before the first LM iteration */
} lvba_window_info;
void lvba_window_default_opts(lvba_window_opts *opts);
int32_t lvba_window_ba(lvba_scans_t scans, const double *poses, const lvba_window_opts *opts, double *window_poses,
                       double *rel_poses, int32_t *anchor_index, double *anchor_poses, int32_t *n_anchors,
                       lvba_scans_t *anchor_scans, lvba_window_info *win_info);
/* The window stage over several GPUs of one node (or several shares on one GPU): the windows are independent problems
 * (src/lvba_system.cpp:232 solves them one after the other), so share k -- scans[k], on whatever device it was created on --
 * holds a contiguous run of whole windows of the sequence (every share but the last a multiple of window_size frames;
 * lvba_window_split gives the frame ranges: frame_begin [n_shares + 1], the thread split of bavoxel.hpp:621-624 applied to
 * windows).  One host thread per share runs lvba_window_ba on it; outputs are those of lvba_window_ba for the concatenated
 * sequence, in window order (poses [n][12] covers all frames); the anchor scan set lives on scans[0]'s device. */
int32_t lvba_window_split(int32_t n_frames, int32_t window_size, int32_t n_shares, int32_t *frame_begin);
int32_t lvba_window_ba_multi(int32_t n_shares, const lvba_scans_t *scans, const double *poses, const lvba_window_opts *opts,
                             double *window_poses, double *rel_poses, int32_t *anchor_index, double *anchor_poses, int32_t *n_anchors,
                             lvba_scans_t *anchor_scans, lvba_window_info *win_info);
/* ---- the whole LiDAR stage -------------------------------------------------------------------------------------------
 *   lvba_lidar_ba <- LvbaSystem::runLidarBA  src/lvba_system.cpp:312-410 (compute only): window BA (or, with
 *   window_enable = 0, every frame its own anchor, :221-229), then for stage 1 (optional) and stage 2 the voxel map of the
 *   anchor clouds at the current anchor poses with that stage's root voxel size and eigen_ratio_array (:356-377) and
 *   damping_iter over all anchors (:386), finally pose_i = anchor(anchor_index_i) o rel_i for every frame (:393-404; frames of
 *   skipped windows keep their input pose).  poses_in / poses_out [n][12] may alias. */
typedef struct {
    lvba_window_opts window;
    int32_t window_enable, stage1_enable;
    double stage_voxel_size[2];
    float stage_eigen_ratio[2][4];
    lvba_balm_opts lm;           /* damping_iter options of the global stages */
} lvba_lidar_ba_opts;
typedef struct {
    int32_t n_frames, n_windows, n_windows_skipped, n_anchors;
    int32_t stage_ran[2], stage_iters[2], stage_status[2], reserved;
    int64_t stage_voxels[2], stage_factors[2];
    double stage_cost_first[2], stage_cost_last[2];
    double window_ms, stage_ms[2];  /* host wall clock */
} lvba_lidar_ba_report;
void lvba_lidar_ba_default_opts(lvba_lidar_ba_opts *opts);
int32_t lvba_lidar_ba(lvba_scans_t scans, const double *poses_in, const lvba_lidar_ba_opts *opts, double *poses_out,
                      lvba_lidar_ba_report *report);
/* The same with the window stage over several GPUs (lvba_window_ba_multi: scans[k] = share k's frames, whole windows, in
 * order; poses_in / poses_out cover all frames): the global stages are single problems over all anchors and run on scans[0]'s
 * device, where the anchor clouds are gathered.  Needs window_enable = 1. */
int32_t lvba_lidar_ba_multi(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in, const lvba_lidar_ba_opts *opts,
                            double *poses_out, lvba_lidar_ba_report *report);

/* The same two calls with pose priors on FRAMES (lvba_balm_set_priors; indices are frame indices of poses_in).  Both global
 * stages apply them to the anchor problem: a frame f of anchor a with rel_f becomes a prior on a with offset rel_f o O, exactly.
 * Priors on frames of skipped windows and relative priors whose two frames share one anchor (constant at this stage) are
 * dropped.  anchor_priors [n_priors] (may be NULL) receives the n_used priors applied, in input order; n_used / n_dropped may be
 * NULL.  The window stage takes no priors.  n_priors = 0: exactly lvba_lidar_ba / lvba_lidar_ba_multi. */
int32_t lvba_lidar_ba_priors(lvba_scans_t scans, const double *poses_in, const lvba_lidar_ba_opts *opts, int32_t n_priors,
                             const lvba_prior *priors, double *poses_out, lvba_lidar_ba_report *report, lvba_prior *anchor_priors,
                             int32_t *n_used, int32_t *n_dropped);
int32_t lvba_lidar_ba_multi_priors(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in, const lvba_lidar_ba_opts *opts,
                                   int32_t n_priors, const lvba_prior *priors, double *poses_out, lvba_lidar_ba_report *report,
                                   lvba_prior *anchor_priors, int32_t *n_used, int32_t *n_dropped);

/* lvba_lidar_ba_multi_priors with robust losses (lvba_balm_set_loss): window_loss on every window problem, stage_loss on both global
 * stages; either may be NULL (none).  The priors stay outside the loss.  Both NULL: exactly lvba_lidar_ba_multi_priors (and with
 * n_shares = 1, n_priors = 0 exactly lvba_lidar_ba).  LVBA_ERR_ARG for an invalid loss, before any work is done. */
int32_t lvba_lidar_ba_robust(int32_t n_shares, const lvba_scans_t *scans, const double *poses_in, const lvba_lidar_ba_opts *opts,
                             const lvba_loss *window_loss, const lvba_loss *stage_loss, int32_t n_priors, const lvba_prior *priors,
                             double *poses_out, lvba_lidar_ba_report *report, lvba_prior *anchor_priors, int32_t *n_used,
                             int32_t *n_dropped);

/* Frame count and per-frame point counts of a scan set; host copy of one frame's xyz [count][3]. */
int32_t lvba_scans_info(lvba_scans_t scans, int32_t *n_frames, int64_t *frame_count);
int32_t lvba_scans_download(lvba_scans_t scans, int32_t frame, float *xyz);

/* ---- The LiDAR map coloured from the camera images (version 112) ----------------------------------------------------------
 *   <- LvbaSystem::VisualizeOptComparison (src/lvba_system.cpp:1932-2144) for one pose set: the after cloud with the refined
 *   scan poses (x_buf_) and cameras (Rcw_all_optimized_), the before cloud with x_buf_before_ and Rcw_all_.
 *   lvba_colorize_create: the handle computes every point of `scans` in the world frame (scan_poses [n_frames][12], R
 *   row-major | t, T_world<-body), stored as float.  scan_times [n_frames] ascending; intr = fx fy cx cy k1 k2 p1 p2; the images
 *   are width x height (the reference's camera size: images of another size are the caller's to resize).
 *   lvba_colorize_add_images: image k (time image_times[k], camera Rcw [k][9] row-major / tcw [k][3] = T_cam<-world, bgr
 *   [k][height][width][3] bytes as cv::imread gives them) takes every point of the scans with |t_scan - t_k| <= half_window_s,
 *   in scan order; an image without points is skipped.  Each point is projected (projectWorldToPixel, std::round, [0,W) x
 *   [0,H)) and a pixel keeps the point the reference's depth buffer keeps (replace when zc + 1e-6f < zbuf, zbuf = (float)zc:
 *   not the nearest one in general), coloured r g b from the pixel.  Kept pixels are merged in row-major order, images in
 *   call order, calls in order.  With leaf_size >= 0.001 the merged cloud is thinned as down_sampling_voxel2 does (per leaf
 *   voxel the first point at the smallest distance to its centre) and comes out sorted by leaf key (x, y, z); otherwise in
 *   merged order.  Images are processed in batches of at most max_batch_images (0: as free device memory allows); the result
 *   does not depend on the batching.
 *   lvba_colorize_count / lvba_colorize_download: the current cloud, xyz [n][3] float and rgb [n][3] bytes.
 *   lvba_colorize_profile: accumulated device time in ms of upload, projection, sort, walk, compaction and thinning.
 *   LVBA_ERR_ARG: null pointers, width or height < 2, scan times not ascending, non-finite poses, times or intrinsics, or (when
 *   thinning) a finite world point more than 2^20 leaves from the origin; the handle stays valid / destroyable. */
typedef struct lvba_colorize_s *lvba_colorize_t;
typedef struct lvba_colorize_opts {
    double half_window_s;     /* scan window around an image time (reference: 0.5 s) */
    double leaf_size;         /* down_sampling_voxel2 leaf (reference: filter_size_points3D = 0.01); < 0.001: no thinning */
    int32_t max_batch_images; /* 0: by free device memory */
    int32_t reserved;
} lvba_colorize_opts;
void lvba_colorize_default_opts(lvba_colorize_opts *o);
int32_t lvba_colorize_create(lvba_scans_t scans, const double *scan_poses, const double *scan_times, const double intr[8],
                             int32_t width, int32_t height, const lvba_colorize_opts *o, lvba_colorize_t *out);
int32_t lvba_colorize_add_images(lvba_colorize_t h, int32_t n, const double *image_times, const double *Rcw, const double *tcw,
                                 const uint8_t *bgr);
int32_t lvba_colorize_count(lvba_colorize_t h, int64_t *n_points);
int32_t lvba_colorize_download(lvba_colorize_t h, float *xyz, uint8_t *rgb);
int32_t lvba_colorize_profile(lvba_colorize_t h, double ms[6]);
void lvba_colorize_destroy(lvba_colorize_t h);

/* ---- Map quality without ground truth: mean map entropy, mean plane variance, normals (version 112) ----------------------
 *   The measures of Razlaw et al. 2015 on the aggregated cloud, plus what the same reduction gives per point.
 *   Cloud: from scans, frames [frame_begin, frame_begin + n_frames) at scan_poses [n_frames][12] (R row-major | t,
 *   T_world<-body; relative to frame_begin as for the voxel maps), every point w = (float)(R (double)p + t) in cloud order (frames
 *   in order, points in scan order) -- the world points of the coloured map --; or n caller-supplied points xyz [n][3] float
 *   (host memory) on `device`.  A non-finite point keeps its index, is nobody's neighbour and, as a query, has count 0.
 *   Queries: the points with index k * query_stride, n_queries = ceil(n_points / query_stride); neighbours: all points.
 *   Neighbourhood of query k: the points j with d2 <= radius * radius, d = (double)w_j - (double)w_k,
 *   d2 = (dx dx + dy dy) + dz dz rounded as written (no fused multiply-add), k itself included; count = their number.
 *   Moments about the query, in fp64: m = sum d / count, S = sum d d^T / count - m m^T.  A query is valid when
 *   count >= min_neighbors and det S (the product of the eigenvalues of S) is finite and > 0; then
 *   entropy = 1/2 ln((2 pi e)^3 det S), plane_var = the smallest eigenvalue, normal = its unit eigenvector, signed so that its
 *   largest component in magnitude is positive; otherwise the three are NaN.
 *   Summary: mme / mpv = the mean entropy / plane_var over the valid queries (NaN without any), mean_neighbors = the mean count
 *   over the queries with a finite point; every sum runs in a fixed order, two calls give the same bytes.  ms = device time of
 *   the world points (or the upload), sort + cell table, reduction, download.
 *   Per-query outputs, each may be NULL: entropy, plane_var, count [n_queries], normal [n_queries][3].
 *   Options: NULL takes the defaults.
 *   LVBA_ERR_ARG: a null scans, scan_poses, xyz (with n > 0) or summary pointer; radius <= 0 or non-finite;
 *   min_neighbors < 4; query_stride < 1; n < 0 or n >= 2^32; a frame range outside the scans or n_frames < 1; a non-finite
 *   pose; a finite point 2^20 - 1 or more cells (of edge radius (1 + 2^-20)) from the origin on any axis.
 *   LVBA_ERR_NOMEM: the cloud does not fit into the free device memory (about 120 bytes per point). */
typedef struct lvba_mapq_opts {
    double radius;         /* neighbourhood radius in metres (default 0.3) */
    int32_t min_neighbors; /* a query with fewer neighbours is invalid (default 8; at least 4) */
    int32_t query_stride;  /* every query_stride-th point is a query (default 1) */
} lvba_mapq_opts;
typedef struct lvba_mapq_summary {
    int64_t n_points, n_queries, n_valid;
    double mme, mpv, mean_neighbors;
    double ms[4];
} lvba_mapq_summary;
void lvba_mapq_default_opts(lvba_mapq_opts *o);
int32_t lvba_mapq_scans(lvba_scans_t scans, const double *scan_poses, int32_t frame_begin, int32_t n_frames,
                        const lvba_mapq_opts *o, lvba_mapq_summary *summary, double *entropy, double *plane_var, float *normal,
                        int32_t *count);
int32_t lvba_mapq_points(int32_t device, int64_t n, const float *xyz, const lvba_mapq_opts *o, lvba_mapq_summary *summary,
                         double *entropy, double *plane_var, float *normal, int32_t *count);

/* ---- scan-to-map registration: point-to-plane Gauss-Newton of scans against a voxel plane map -------------
 *   A batch of n independent jobs; job k registers frame frames[k] of `scans` from the pose poses[k] (R row-major | t,
 *   T_world<-body) against `map`.  The map and the scans may come from different scan sets (relocalisation) but lie on one device.
 *   Per point p of the frame (fp32, promoted once), all in fp64 and rounded as written (no fused multiply-add):
 *     w = (R00 px + R01 py) + R02 pz + tx, ...     the world point
 *     (n, d)                                        its plane, exactly as lvba_voxmap_find_planes associates it
 *     r = (n0 w0 + n1 w1) + n2 w2 + d               inlier iff a plane was found and |r| <= max_distance
 *     J = [ p x (R^T n) ; n ]                       d r / d(theta, t) under the retraction R <- R Exp(theta), t <- t + delta
 *     H += rho' J J^T, g += rho' J r, cost += rho   with (rho, rho') = loss(r^2), scale in metres (first-order IRLS weights);
 *                                                   no loss: rho = r^2, rho' = 1
 *   lvba_register_linearize returns these sums at the given poses: H [n][36] (full, symmetric, tangent order (theta, t)),
 *   g [n][6], cost [n], inliers [n].
 *   lvba_register_scans iterates every job, in lock-step on the device, until each has a status:
 *     LVBA_REG_TOO_FEW_INLIERS   inliers < max(min_inliers, 1); the pose stays as it is
 *     LVBA_REG_DEGENERATE        the smallest eigenvalue of H / inliers is below min_eigenvalue (or H has no LDL^T with positive
 *                                pivots); the pose stays as it is
 *     LVBA_REG_CONVERGED         delta = -H^-1 g has |dtheta| <= tol_rot and |dt| <= tol_pos; this last step is not applied, so
 *                                the information and the statistics belong to the returned pose
 *     LVBA_REG_MAX_ITERATIONS    max_iterations linearisations were taken, each followed by its step
 *   poses_out [n][12]; information [n][36] = H at the job's last linearisation; results[k]: status, iterations (linearisations
 *   taken), inliers / cost_last / rmse = sqrt(cost_last / inliers) / min_eigenvalue of the last linearisation, cost_first of the
 *   first, points = the frame's point count.  Every sum runs in a fixed order that depends on the job's point count alone: two
 *   calls give the same bytes, and a job gives the same bytes whatever else is in the batch.
 *   An empty map is not an error: every job ends LVBA_REG_TOO_FEW_INLIERS.  Options: NULL takes the defaults.
 *   LVBA_ERR_ARG: a null pointer (with n > 0), n < 0, a frame outside the scans, a non-finite pose, map and scans on different
 *   devices, max_iterations outside 1 .. 1000, max_distance not finite and > 0, a negative min_inliers, min_eigenvalue or tolerance,
 *   an unknown loss kind or a non-trivial loss whose scale is not finite and > 0.
 *   LVBA_ERR_UNSUPPORTED: a joint map of several windows or a view into one (as lvba_voxmap_find_planes). */
#define LVBA_REG_CONVERGED 0
#define LVBA_REG_MAX_ITERATIONS 1
#define LVBA_REG_TOO_FEW_INLIERS 2
#define LVBA_REG_DEGENERATE 3
typedef struct lvba_register_opts {
    int32_t max_iterations; /* default 30 */
    double max_distance;    /* inlier gate on |r| in metres (default 0.1) */
    int64_t min_inliers;    /* default 100 */
    double min_eigenvalue;  /* of H / inliers (default 1e-3) */
    double tol_rot, tol_pos; /* rad, m (default 1e-6 each) */
    lvba_loss loss;         /* default LVBA_LOSS_TRIVIAL */
} lvba_register_opts;
typedef struct lvba_register_result {
    int32_t status, iterations;
    int64_t inliers, points;
    double cost_first, cost_last, rmse, min_eigenvalue;
} lvba_register_result;
void lvba_register_default_opts(lvba_register_opts *o);
int32_t lvba_register_linearize(lvba_voxmap_t map, lvba_scans_t scans, int32_t n, const int32_t *frames, const double *poses,
                                const lvba_register_opts *o, double *H, double *g, double *cost, int64_t *inliers);
int32_t lvba_register_scans(lvba_voxmap_t map, lvba_scans_t scans, int32_t n, const int32_t *frames, const double *poses_init,
                            const lvba_register_opts *o, double *poses_out, double *information, lvba_register_result *results);

/* ---- submap sets: many submaps in one map, a key lookup per submap ------------------------------------------
 *   lvba_submaps_build cuts frames [frame_begin, frame_begin + n_frames) of `scans` into submaps of submap_size frames -- submap
 *   w holds frames [frame_begin + w S, min(frame_begin + (w + 1) S, frame_begin + n_frames)); the last one may be ragged -- and
 *   builds all of them in ONE pass at poses [n_frames][12]: every submap's roots and planes are, bit for bit, those of
 *   lvba_voxmap_build_scans on its own frames.  The handle is a voxel map on a stream of its own: lvba_voxmap_info gives the
 *   totals, lvba_voxmap_destroy frees it.  submap_size >= n_frames gives one submap (a plain map); a plain map built by
 *   lvba_voxmap_build* is accepted wherever a submap set is, as a set of one submap.
 *   lvba_submaps_count: the number of submaps and their size in frames.
 *   lvba_submaps_find_planes: lvba_voxmap_find_planes with one submap index per point; point i is looked up among the planes of
 *   submap[i] only.  An index outside 0 .. n_submaps - 1 gives valid = 0 (and a zero plane), not an error.
 *   lvba_register_linearize_submaps / lvba_register_scans_submaps: lvba_register_linearize / lvba_register_scans where job k
 *   associates its points with the planes of submap submap[k] only.  Arithmetic, statuses and summation order are those of the
 *   single-map calls: a job gives the bytes lvba_register_scans gives on the submap's own map, whatever else is in the batch.  A
 *   submap without planes ends its jobs LVBA_REG_TOO_FEW_INLIERS.
 *   LVBA_ERR_ARG: as the single-map calls, and a submap index outside 0 .. n_submaps - 1 in a registration job, submap_size < 1.
 *   LVBA_ERR_UNSUPPORTED: a view into a joint map.  lvba_voxmap_find_planes, lvba_register_linearize and lvba_register_scans
 *   keep refusing a set of several submaps (LVBA_ERR_UNSUPPORTED): they have no submap to search. */
int32_t lvba_submaps_build(lvba_scans_t scans, int32_t frame_begin, int32_t n_frames, int32_t submap_size, const double *poses,
                           const lvba_voxel_opts *opts, lvba_voxmap_t *out);
int32_t lvba_submaps_count(lvba_voxmap_t submaps, int32_t *n_submaps, int32_t *submap_size);
int32_t lvba_submaps_find_planes(lvba_voxmap_t submaps, int64_t n, const int32_t *submap, const double *X, double *plane,
                                 uint8_t *valid);
int32_t lvba_register_linearize_submaps(lvba_voxmap_t submaps, lvba_scans_t scans, int32_t n, const int32_t *frames,
                                        const int32_t *submap, const double *poses, const lvba_register_opts *o, double *H, double *g,
                                        double *cost, int64_t *inliers);
int32_t lvba_register_scans_submaps(lvba_voxmap_t submaps, lvba_scans_t scans, int32_t n, const int32_t *frames,
                                    const int32_t *submap, const double *poses_init, const lvba_register_opts *o, double *poses_out,
                                    double *information, lvba_register_result *results);

/* ---- loop-closure candidates: which frame revisits which submap, from the poses alone -----------------------
 *   poses [n_frames][12] (R row-major | t); only t is read.  With S = submap_size, submap w holds frames
 *   F_w = [w S, min((w + 1) S, n_frames)).  A query frame j is a multiple of query_stride.  Every squared distance is
 *     d2(j, f) = ((dx dx + dy dy) + dz dz),  dx = tx_j - tx_f, ...       in fp64, rounded as written (no fused multiply-add)
 *   (j, w) is eligible iff |j - f| >= min_gap for EVERY f in F_w, and min over F_w of d2(j, f) <= radius * radius.
 *   ref is the f in F_w with the smallest d2; on a tie the lowest f.  Per query the max_per_frame eligible submaps with the
 *   smallest d2 are kept; on a tie the lower w.  The output is sorted by (query, submap); distance = sqrt(d2).
 *   *count is the true number of candidates even when it exceeds capacity; only the first `capacity` are written.
 *   No atomics: two calls give the same bytes.  n_frames = 0 gives *count = 0.  Options: NULL takes the defaults with
 *   submap_size 10.
 *   LVBA_ERR_ARG: a null pointer, n_frames < 0, capacity < 0, a non-finite pose, submap_size < 1, min_gap < 0, max_per_frame
 *   outside 1 .. 32, query_stride < 1, radius not finite and > 0. */
typedef struct lvba_loop_opts {
    int32_t submap_size;     /* S >= 1 (default 10) */
    int32_t min_gap;         /* frames (default 50) */
    int32_t max_per_frame;   /* 1 .. 32 (default 2) */
    int32_t query_stride;    /* >= 1 (default 1) */
    double radius;           /* metres, finite and > 0 (default 5) */
} lvba_loop_opts;
typedef struct lvba_loop_candidate {
    int32_t query, submap, ref;
    int32_t pad;
    double distance;
} lvba_loop_candidate;
void lvba_loop_default_opts(lvba_loop_opts *o);
int32_t lvba_loop_candidates(int32_t device, int32_t n_frames, const double *poses, const lvba_loop_opts *o, int64_t capacity,
                             lvba_loop_candidate *out, int64_t *count);

/* ---- place recognition: which frame revisits which submap, from the clouds alone (Scan Context) ---------------
 *   Descriptor of a frame, Nr = n_rings, Ns = n_sectors.  Every body-frame point (x, y, z), fp32 promoted once to fp64:
 *     r = sqrt(x x + y y); the point is dropped unless min_range <= r < max_range (a non-finite x or y drops it)
 *     ring   = min(floor((r Nr) / max_range), Nr - 1)
 *     sector = min(floor(((atan2(y, x) + pi) Ns) / (2 pi)), Ns - 1)      atan2 in fp64, pi = 3.14159265358979323846; a point within
 *                                                                          an ulp or two of a sector boundary may fall either side
 *     h = (float)(z + z_offset); a point whose h is not finite is dropped
 *     D[ring][sector] = max(0, max of h over the cell's points)         fp32; an empty cell is 0.  A maximum: the same bytes
 *                                                                          however it is reduced
 *   Ring key: key[ring] = (float)((double)(number of sectors with D > 0) / (double)Ns); it does not change when the body turns
 *   about z.  Normalised columns: U[:, j] = D[:, j] / sqrt(sum over ring of D[ring][j]^2), fp64, the sum in ring order; a zero
 *   column stays zero and is "empty".
 *   Shift distance of query q against frame c, for s = 0 .. Ns - 1:
 *     sim(s) = sum over j, then ring, of U_q[ring][(j - s) mod Ns] U_c[ring][j]   over the columns j where neither side is empty, in
 *              (j, ring) order, fp64, rounded as written (no fused multiply-add); n(s) = the number of such columns
 *     dist(s) = 1 - sim(s) / n(s), or 1 when n(s) = 0;   distance = min over s, shift = the smallest s that attains it
 *     yaw = (2 pi shift) / Ns, minus 2 pi when above pi
 *   T_c o (Rz(yaw), 0) is then the initial T_world<-body of q: the body of q is the body of c turned by yaw about its own z.
 *   Candidates, with S = submap_size and submap w = frames F_w = [w S, min((w + 1) S, n)): a query j (a multiple of query_stride)
 *   considers the frames f of the submaps with |j - f'| >= min_gap for EVERY f' in F_w.  Among them the K = n_key_candidates
 *   smallest (sum over ring of (key_j - key_f)^2, f) pairs -- the sum in fp32, in ring order, rounded as written; the order
 *   lexicographic -- are kept and the shift distance is computed for exactly these.  Per submap with at least one of the K, ref
 *   is the frame of the smallest (distance, f); the submap is eligible iff that distance <= max_distance.  Per query the
 *   max_per_frame eligible submaps of the smallest (distance, w) are kept.  The output is sorted by (query, submap).
 *   *count is the true number of candidates even when it exceeds capacity; only the first `capacity` are written.  No
 *   floating-point atomics, every sum and minimum in a fixed order: two calls give the same bytes.
 *   lvba_place_descriptors: desc [n_frames][Nr][Ns] and ring_key [n_frames][Nr] of frames [frame_begin, frame_begin + n_frames).
 *   lvba_place_search: the candidates among n_frames descriptors from anywhere (the ring keys are derived from desc).
 *   lvba_place_candidates: both over all frames of `scans`, the descriptors staying on the device; the bytes of the composition.
 *   A frame without points has an all-zero descriptor; its distance to anything is 1.  n_frames = 0 gives *count = 0.  Options:
 *   NULL takes the defaults.
 *   LVBA_ERR_ARG: a null pointer, a frame range outside the scans, n_frames < 0, capacity < 0, an option outside its range below,
 *   a descriptor value given to lvba_place_search that is not finite and >= 0. */
typedef struct lvba_place_opts {
    int32_t n_rings;          /* Nr, 1 .. 32 (default 20) */
    int32_t n_sectors;        /* Ns, 1 .. 128 (default 60) */
    double min_range;         /* metres, finite and >= 0 (default 0.5) */
    double max_range;         /* metres, finite and > min_range (default 80) */
    double z_offset;          /* metres, finite (default 2) */
    int32_t submap_size;      /* S >= 1 (default 10) */
    int32_t min_gap;          /* frames, >= 0 (default 50) */
    int32_t n_key_candidates; /* K, 1 .. 32 (default 10) */
    int32_t max_per_frame;    /* 1 .. 32 (default 2) */
    int32_t query_stride;     /* >= 1 (default 1) */
    int32_t pad;
    double max_distance;      /* in (0, 1] (default 0.4) */
} lvba_place_opts;
typedef struct lvba_place_candidate {
    int32_t query, submap, ref, shift;
    double distance, yaw;
} lvba_place_candidate;
void lvba_place_default_opts(lvba_place_opts *o);
int32_t lvba_place_descriptors(lvba_scans_t scans, int32_t frame_begin, int32_t n_frames, const lvba_place_opts *o,
                               float *desc, float *ring_key);
int32_t lvba_place_search(int32_t device, int32_t n_frames, const float *desc, const lvba_place_opts *o, int64_t capacity,
                          lvba_place_candidate *out, int64_t *count);
int32_t lvba_place_candidates(lvba_scans_t scans, const lvba_place_opts *o, int64_t capacity, lvba_place_candidate *out,
                              int64_t *count);

/* ---- pairwise consistency of loop closures: voting out a closure that contradicts the others -----------------
 *   After Mangelson et al., "Pairwise Consistent Measurement Set Maximization", ICRA 2018, with fixed tolerances in place of the
 *   Mahalanobis test (the project has no odometry covariance to put in one).
 *   A closure k = (i_k = ref[k], j_k = query[k], Z_k = meas[k]): Z_k is the measured T_i^-1 T_j, 12 doubles, R row-major then t --
 *   the `meas` of an LVBA_PRIOR_RELATIVE prior between ref and query.  poses [n_frames][12] are the current (possibly drifted)
 *   poses X; their local relative motion is trusted.  X_pq = X_p^-1 X_q.
 *   Cycle of two closures a < b (positions in the caller's list):
 *     E_ab = Z_a . X_{j_a j_b} . Z_b^-1 . X_{i_b i_a}        the identity if both closures and the odometry agree; in the frame of i_a
 *     rot_ab = |Log(R_E)|, the angle atan2(|vee(R_E - R_E^T)| / 2, (tr R_E - 1) / 2);   trans_ab = |t_E|
 *     L_ab = |j_a - j_b| + |i_a - i_b|                          the odometry steps in the cycle
 *   The pair is consistent iff rot_ab <= rot_tol + rot_rate L_ab and trans_ab <= trans_tol + trans_rate L_ab (the right-hand sides
 *   in fp64, rounded as written).  The pair (b, a) takes the decision and the two values of (a, b): the matrix is exactly
 *   symmetric.  A closure is consistent with itself; rot_aa = trans_aa = 0.  The odometry legs run from ref to ref and from query
 *   to query: closures that are to agree must name their frames in the same order (the earlier frame as ref, say), and (j, i,
 *   Z^-1) is to be given for (i, j, Z) where they do not.  The values are computed from the prepared form
 *   P_k = X_j Z_k^-1 X_i^-1, E_ab = X_{i_a}^-1 P_a^-1 P_b X_{i_a}, and agree with the six compositions above to rounding.
 *   adjacency [n][W] of uint64_t, W = ceil(n / 64): bit (b mod 64) of word adjacency[a][b / 64] is the decision; the diagonal is
 *   set; bits at positions >= n are zero.
 *   The set: deg(v) = popcount(A[v]) - 1.  The seeds are the first min(n_seeds, n) closures by (deg descending, index ascending).
 *   For seed s: K = {s}, C = A[s] \ {s}; while C is not empty, pick the v in C with the largest |A[v] & C|, the lowest v on a tie,
 *   and set K <- K + {v}, C <- (C & A[v]) \ {v}.  The result is the largest K, on a tie the one of the seed that comes first in
 *   seed order; keep[k] = 1 for its members and *n_keep their number.  If it has fewer than min_set members nothing is kept.
 *   Every K is a clique by construction.  The search is a greedy heuristic: it is NOT guaranteed to find the maximum clique.
 *   (A seed stops early when every vertex of C has |A[v] & C| = |C|: C is then a clique and the rule would take all of it.  This
 *   does not change the result.)
 *   No atomics, every maximum lexicographic with a fixed tie rule: two calls give the same bytes.  n = 0 gives *n_keep = 0.
 *   Options: NULL takes the defaults, which are a judgement and not a measurement on real data.  adjacency, rot, trans may be
 *   NULL; rot and trans are diagnostics of n * n doubles each.
 *   LVBA_ERR_ARG: a null required pointer, n < 0 or n > 16384 (the adjacency is then 32 MB, a candidate set 2 KB of LDS),
 *   n_frames < 1 with n > 0, an index outside the frames, ref == query, a non-finite pose or measurement, a measurement rotation
 *   that is not orthonormal within 1e-6, an option outside its range.  A refused call writes nothing. */
typedef struct lvba_closure_opts {
    double rot_tol;     /* rad, finite and >= 0 (default 0.035) */
    double rot_rate;    /* rad per frame, finite and >= 0 (default 0.001) */
    double trans_tol;   /* metres, finite and >= 0 (default 0.2) */
    double trans_rate;  /* metres per frame, finite and >= 0 (default 0.01) */
    int32_t n_seeds;    /* >= 1 (default 32), clamped to n */
    int32_t min_set;    /* >= 1 (default 2) */
} lvba_closure_opts;
void lvba_closure_default_opts(lvba_closure_opts *o);
int32_t lvba_closure_consistency(int32_t device, int32_t n_frames, const double *poses, int32_t n, const int32_t *ref,
                                 const int32_t *query, const double *meas, const lvba_closure_opts *o, uint64_t *adjacency,
                                 double *rot, double *trans, uint8_t *keep, int32_t *n_keep);

/* Pose-graph relaxation over odometry and loop closures (opt-in).  One call, no handle.
 *   Poses X [n_poses][12] (R row-major | p) move under BALM's retraction R <- R Exp(dphi), p <- p + dp, d = [phi; p].  Minimised:
 *     C(x) = sum_{i=0..N-2} 1/2 |L_o r(X_i, X_{i+1}; Z0_i)|^2 + sum_k 1/2 rho(|L_k r_k(x)|^2) + 1/2 |L_a r_pose(X_a; X0_a)|^2
 *   r       the LVBA_PRIOR_RELATIVE residual above (rotation first, offsets honoured), r_pose the LVBA_PRIOR_POSE residual.
 *   odometry  edge i keeps the relative motion of the INPUT poses, Z0_i = X0_i^-1 X0_{i+1}, with L_o = diag(1/odom_sigma_rot x 3,
 *           1/odom_sigma_pos x 3).  The sigmas are per frame step and a judgement (a trajectory file has no covariances); only their
 *           ratio to the closures' information moves the result.
 *   closures  the `edges` array: LVBA_PRIOR_RELATIVE only, as find_loop_closures builds them.
 *   anchor  pose `anchor` is held at its input value by L_a = diag(1/anchor_sigma_rot x 3, 1/anchor_sigma_pos x 3).  The rest of C is
 *           gauge-invariant, so at the minimum this residual is zero and the solution does not depend on L_a (finite, > 0).  The
 *           default, 1e-4 rad / 1e-4 m, is stiff: the covariance call's convention is an anchor that does not move, and a stiff
 *           prior keeps the anchor in place during the damped steps too, not only at the minimum.
 *   rho     closure_loss, one of LVBA_LOSS_* with s = |L_k r_k|^2 dimensionless, on the closure edges only; gradient and
 *           Gauss-Newton block are scaled by rho'(s), the rho'' term is left out (as lvba_balm_set_loss).  Default TRIVIAL.
 *   The LM rule (the numpy oracle of the tests and the device driver follow this text):
 *     u = 0.01, v = 2.  H, g, C1 <- the Gauss-Newton system and cost at x ("evaluated").  If the first C1 == 0: stop, no iteration.
 *     Iteration it = 0 .. max_iter - 1:
 *       dx = -(H + u diag(H))^-1 g;  x' = x [+] dx;  q1 = 1/2 dx^T (u diag(H) dx - g);  C2 = C(x');  q = C1 - C2.
 *       A flagged pivot makes q NaN (status LVBA_NUM_FACTORIZATION), a non-finite C2 gives status LVBA_NUM_NONFINITE.
 *       q > 0 (accepted):  x <- x';  t = 1 - (2 q / q1 - 1)^3;  u <- u * max(1/3, t);  v <- 2;  H, g, C1 are evaluated again at
 *                          the new x;  if q / C1(old) < rel_tol: stop after this iteration.
 *       else (rejected):   u <- u v;  v <- 2 v;  H, g, C1 are kept.
 *     The trace row of an iteration holds residual1 = C1, residual2 = C2 (sums, not averages), u, v as used, q, q1.
 *   poses_out [n_poses][12] receives the result; edge_weight [n_edges] (may be NULL) rho'(s_k) at the result; trace (may be NULL)
 *   needs room for max_iter rows, *n_trace (may be NULL) their number; report is required.  report.solver_kind: LVBA_PG_SOLVER_*,
 *   which form of the damped solve the graph was given (-1: nothing was solved); cost_last = C at the result, odom_cost_last and
 *   closure_cost_last its first two sums; max_step_last = max |dx| of the last accepted step (0 if none).
 *   n_edges = 0 is legal: the cost is 0, nothing is launched, poses_out equals poses byte for byte.
 *   LVBA_ERR_ARG (every output untouched): a null required pointer, n_poses < 2, n_edges < 0, an edge that is not RELATIVE, an index
 *   out of range, i == j, a non-finite value or a rotation (pose, measurement, offset) that is not orthonormal within 1e-6, a sigma
 *   or rel_tol that is not finite and > 0, max_iter < 0, a bad loss, an anchor outside the poses.
 *   LVBA_NUM_FACTORIZATION / LVBA_NUM_NONFINITE: as lvba_balm_refine -- the iteration is a rejected step, the loop goes on, the
 *   worst status is returned at the end and the outputs are written.  lvba_version() is unchanged; look the symbols up. */
#define LVBA_PG_SOLVER_BAND 0
#define LVBA_PG_SOLVER_DISSECTED 1
#define LVBA_PG_SOLVER_DENSE 2
typedef struct lvba_posegraph_opts {
    int32_t anchor, max_iter;           /* 0, 50 */
    double odom_sigma_rot, odom_sigma_pos, anchor_sigma_rot, anchor_sigma_pos, rel_tol; /* 0.01 rad, 0.05 m, 1e-4, 1e-4, 1e-6 */
    lvba_loss closure_loss;             /* TRIVIAL */
} lvba_posegraph_opts;
typedef struct lvba_posegraph_report {
    int32_t iterations, accepted, status, solver_kind /* band / dissected / dense, as lvba_balm_info names them */;
    double cost_first, cost_last, odom_cost_last, closure_cost_last, max_step_last;
} lvba_posegraph_report;
void    lvba_posegraph_default_opts(lvba_posegraph_opts *);
int32_t lvba_posegraph_relax(int32_t n_poses, const double *poses, int32_t n_edges, const lvba_prior *edges,
                             const lvba_posegraph_opts *opts, int32_t device, double *poses_out,
                             double *edge_weight /* [n_edges] rho'(s) at the result, may be NULL */,
                             lvba_lm_trace *trace, int32_t *n_trace /* may be NULL */,
                             lvba_posegraph_report *report);

/* ---- descriptor matching of image pairs, with an optional pose-guided gate: epipolar or through LiDAR depth (opt-in)
 *   The reference's fallback when its COLMAP database holds no verified matches (src/lvba_system.cpp:697-833) matches every image
 *   pair with SiftMatchGPU::GetSiftMatch(n, buf, 0.7f, 0.8f, 1).  SiftGPU's source is not part of the reference tree: the rule
 *   below is this project's own definition of those three documented parameters, restated by a numpy oracle and NOT pinned against
 *   SiftGPU.
 *   Descriptor: 128 uint8 values (nominal norm 512, as SiftGPU and COLMAP store them; nothing is assumed about the actual norm).
 *   Image i has n_i >= 0 of them, at most 1 048 576.
 *   Score  s(r, c) = sum_k a_r[k] b_c[k], an exact integer (< 2^23).   Distance  d = acos(min(s / 262144, 1)), in fp64.
 *   Top two of row r of the ORDERED pair (a, b), over the columns that take part (all of b; under the gate those that pass it):
 *     best(r) = the column of the largest score, the lowest column on a tie;  s1 = that score;
 *     s2 = the largest score over the other columns, 0 when there is no other column (d2 = pi / 2).  A duplicate of the best column
 *     gives s2 = s1.  A row with no column at all has best = -1, s1 = s2 = 0.
 *   (r, c) is a match of the pair (a, b) iff  c = best_ab(r) >= 0,  d1 < max_distance,  d1 < max_ratio * d2 (the product in fp64,
 *   rounded as written)  and, if mutual, best_ba(c) = r -- the same rule with the images swapped, under the gate with the same gate.
 *   The distance and the mutual clause are symmetric in the two images, the ratio clause is not (d2 is the second best of the
 *   row's own image): the matches of (b, a) are the transposed matches of (a, b) only where the ratio clause passes on both sides.
 *   The matches of a pair are listed by ascending r, the pairs in the caller's order.  acos is the device's fp64 acos: a d1 within
 *   an ulp or two of a bound may fall either side.
 *   Guided gate (guided = 1, needs lvba_match_set_geometry).  Keypoints (u, v) are fp32 pixels; x^ = (x, y, 1) is the undistorted
 *   normalised point (the reference's undistortPixelToNormalized, include/utils.hpp, fp64).  A keypoint whose undistortion fails
 *   matches nothing under the gate, in any pair.  Cameras are T_cam<-world = (R, t), the visual stage's convention.  With lo the
 *   image of the pair with the smaller index and hi the other:
 *     R_lh = R_hi R_lo^T,  t_lh = t_hi - R_lh t_lo,  E = [t_lh]x R_lh               every sum left to right, no fused multiply-add
 *     for a keypoint p of lo and a keypoint q of hi:
 *       l = E x^_p,  n_lo = l0 l0 + l1 l1;    l' = E^T x^_q,  n_hi = l'0 l'0 + l'1 l'1;    e = (x_q l0 + y_q l1) + l2
 *       the candidate passes iff  e e <= tau^2 (n_lo + n_hi)   (the Sampson distance),  tau = (2 max_epipolar_px) / (fx + fy)
 *   The ordered pairs (lo, hi) and (hi, lo) evaluate these same expressions on the same operands (E of (hi, lo) is E^T): the
 *   decision for (r, c) in one is bit for bit the decision for (c, r) in the other.  A pair whose centres coincide,
 *   |t_lh|^2 <= 1e-20 (|t_lo|^2 + |t_hi|^2), has no epipolar geometry: E is taken as zero and every candidate (of keypoints whose
 *   undistortion succeeded) passes.
 *   Depth-guided gate (guided = 2, needs lvba_match_set_geometry and then lvba_match_set_depth).  An epipolar gate cannot separate
 *   copies of a texture that lie along the epipolar line; a keypoint with a LiDAR depth return is a 3-D point, and its image in
 *   the other view is a point, not a line.
 *     The point of keypoint p of image i, fp32 pixel (u, v):  d = fetchDepthBilinear(depth_i, u, v)  (float arithmetic, all four
 *       neighbours > 0, exactly as lvba_fuse_tracks samples it);  X^c = (x d, y d, d) with (x, y) the undistorted normalised point
 *       above;  X_p = camToWorld(X^c) = R_i^T X^c + (-(R_i^T t_i)), every sum left to right, no fused multiply-add (the expressions
 *       of the track fusion).  p HAS A POINT iff the fetch and the undistortion succeed and X^c and X_p are finite.
 *     The prediction of p in image j:  (u^, v^) = the distorted pixel of X_p under (R_j, t_j) (the reference's
 *       projectCameraToPixel).  When the projection fails (Z <= 1e-12 or a non-finite value) the prediction is NOWHERE.
 *     For a keypoint q of image j with pixel (u_q, v_q) widened to fp64:  d2(p -> q) = (u_q - u^)(u_q - u^) + (v_q - v^)(v_q - v^).
 *     The candidate (p, q) passes iff  at least one of p, q has a point,  and for each of the two that has a point
 *       d2 <= rho rho,  rho = max_reproj_px  -- false for a NaN pixel and for a prediction that is nowhere.
 *   If neither keypoint has a point the candidate fails: a caller who wants those keypoints matched runs guided = 1 on them.
 *   There is no occlusion test (the point of p may be hidden in j): the descriptor decides.  As under the epipolar gate, both
 *   orientations of a pair evaluate these same expressions on the same operands: the decision for (r, c) in (a, b) is bit for bit
 *   the decision for (c, r) in (b, a), as the mutual clause requires.  max_reproj_px defaults to 8, twice the epipolar default; no
 *   real dataset was at hand to choose it on.
 *   lvba_match_create: desc_off [n_images + 1] (desc_off[0] = 0), desc [sum n][128]; the descriptors go to the device once.
 *   lvba_match_set_geometry: keypoints_uv [sum n][2] in descriptor order, intr = (fx, fy, cx, cy, k1, k2, p1, p2), Rcw [n_images][9]
 *   row-major, tcw [n_images][3]; undistorts on the device once; may be called again (new poses replace the old, and the lifted
 *   points are dropped: they were lifted with the old poses).
 *   lvba_match_set_depth: lifts every keypoint of every image once, on the device, into a resident [sum n][3] fp64 table (NaN rows:
 *   no point).  depth: one image per image of the matcher (lvba_depth_render / lvba_depth_upload), on the matcher's device; it is
 *   only read during the call.  depth = NULL drops the table.  lvba_match_points downloads the table, world [sum n][3].
 *   lvba_match_pairs: all pairs in one call, their work tiled over one grid per 2^23 scanned rows.  matches [capacity][2] = (r, c),
 *   scores [capacity] (may be NULL) = s1 of each match, match_off [n_pairs + 1] the first match of each pair.  *count is the true
 *   number of matches and match_off the true offsets even when they exceed capacity; only the first `capacity` matches are
 *   written.  lvba_match_scan: best, s1, s2 [n_a] of the ordered pair (a, b) before any threshold (it reads only guided,
 *   max_epipolar_px and max_reproj_px of the options).  No atomics: two calls give the same bytes.  Options: NULL takes the defaults.
 *   LVBA_ERR_ARG: a null required pointer, a negative count, desc_off that does not start at 0 or decreases, an image above the
 *   per-image limit, a pair index outside the images, a == b, an option outside its range below (non-finite included), guided
 *   without geometry, guided = 2 or lvba_match_points without lifted points, lvba_match_set_depth without geometry or with a depth
 *   set of another image count or on another device, non-finite intrinsics or poses, fx or fy <= 0, a rotation that is not orthonormal within 1e-6 with
 *   determinant > 0.  A refused call writes nothing (a refused set_geometry keeps the geometry and the points it had, a refused set_depth the
 *   points).  lvba_match_opts grew by max_reproj_px (32 -> 40 bytes) with these two calls; lvba_version() is unchanged, a client
 *   detects the larger struct by looking lvba_match_set_depth up. */
typedef struct lvba_match_s *lvba_match_t;
typedef struct lvba_match_opts {
    double max_distance;     /* rad, finite and > 0 (default 0.7) */
    double max_ratio;        /* in (0, 1] (default 0.8) */
    int32_t mutual;          /* 0 or 1 (default 1) */
    int32_t guided;          /* 0 none, 1 epipolar, 2 depth (default 0) */
    double max_epipolar_px;  /* pixels, finite and > 0 (default 4) */
    double max_reproj_px;    /* pixels, finite and > 0 (default 8); checked always, used by guided = 2 */
} lvba_match_opts;
void    lvba_match_default_opts(lvba_match_opts *o);
int32_t lvba_match_create(int32_t device, int32_t n_images, const int64_t *desc_off, const uint8_t *desc, lvba_match_t *out);
int32_t lvba_match_destroy(lvba_match_t m);
int32_t lvba_match_set_geometry(lvba_match_t m, const float *keypoints_uv, const double *intr, const double *Rcw, const double *tcw);
int32_t lvba_match_pairs(lvba_match_t m, int64_t n_pairs, const int32_t *pairs, const lvba_match_opts *o, int64_t capacity,
                         int32_t *matches, int32_t *scores, int64_t *match_off, int64_t *count);
int32_t lvba_match_scan(lvba_match_t m, int32_t a, int32_t b, const lvba_match_opts *o, int32_t *best, int32_t *s1, int32_t *s2);
int32_t lvba_match_set_depth(lvba_match_t m, lvba_depth_t depth);
int32_t lvba_match_points(lvba_match_t m, double *world);

/* ---- which image pairs to match, from LiDAR co-visibility (opt-in)
 *   The reference matches all M (M - 1) / 2 image pairs (image_pairs_, src/lvba_system.cpp:462-466).  After the LiDAR stage the
 *   camera poses and one LiDAR depth image per camera are on the device, so "does image j see what image i sees" is a question
 *   about geometry that is already there, occlusion included.  The rule is this project's own; a numpy oracle restates it.
 *   Inputs: a depth set of M images of W x H pixels, Rcw [M][9] row-major and tcw [M][3] (T_cam<-world), intr = (fx, fy, cx, cy,
 *   k1, k2, p1, p2).  Every expression in fp64 unless it says float, every sum left to right, no fused multiply-add.
 *   Samples.  Image i gets G = grid_x grid_y cells, sample s = gy grid_x + gx.  The cell's centre pixel is
 *     px = ((2 gx + 1) (W - 1)) / (2 grid_x),  py = ((2 gy + 1) (H - 1)) / (2 grid_y)   in integer division, so 0 <= px <= W - 2.
 *     Candidates: the centre, then the Chebyshev rings r = 1 .. search_radius around it, each ring walked dy = -r .. r and inside
 *     that dx = -r .. r, keeping only |dx| = r or |dy| = r.  A candidate outside [0, W - 2] x [0, H - 2] is skipped.  The first
 *     candidate (u, v) for which the undistortion of the pixel ((double)(float)u, (double)(float)v) succeeds, the depth image of i
 *     has a return there (fetchDepthBilinear at the float pixel: all four neighbours > 0) and the world point
 *     X = camToWorld((x d, y d, d)) is finite -- the expressions of lvba_fuse_tracks and of the matcher's depth gate -- is the
 *     cell's sample.  If no candidate succeeds the cell HAS NO POINT (a NaN row).  n_i = the cells of image i with a point.  The
 *     search exists because rendered LiDAR depth images have holes.
 *   Seen.  For an ordered pair (i, j), i != j, sample s of i is SEEN IN j iff it has a point, the projection of X under (R_j, t_j)
 *     (projectCameraToPixel: Z > 1e-12, all finite) succeeds, its pixel (u^, v^) has 0 <= u^ < W - 1 and 0 <= v^ < H - 1, and,
 *     with occlusion on, it is not HIDDEN: hidden iff fetchDepthBilinear of depth image j at ((float)u^, (float)v^) succeeds with
 *     depth d and  Z > (double)d * (1.0 + occlusion_rel) + occlusion_abs,  Z = R_j[6] X[0] + R_j[7] X[1] + R_j[8] X[2] + t_j[2].
 *     A fetch that fails is a hole in j: no evidence of occlusion, the sample counts as seen.
 *     c_ij = the samples of i seen in j;  c_ii = 0.
 *   Score.  r_ij = c_ij / n_i (0 when n_i = 0).  For i < j: score = max(r_ij, r_ji), shared = max(c_ij, c_ji); with both_ways
 *     both take the min.  The pair is ELIGIBLE iff shared >= min_shared and score >= min_overlap.
 *   Cap.  With max_per_image = K > 0 the partners of image i among its eligible pairs are ranked by (score descending, partner
 *     index ascending); an eligible pair is kept iff its partner rank is < K for i or for j.  K = 0 keeps every eligible pair.
 *   Output: the kept pairs (i, j), i < j, sorted by (i, j); score [capacity] and shared [capacity][2] = (c_ij, c_ji) may be NULL.
 *   *count is the true number even above capacity; only the first `capacity` entries are written.  No atomics: two calls give the
 *   same bytes.  The three calls run on the depth set's device and only read it; each lifts the samples itself.
 *   The samples call gives world [M][G][3], the counts call n_points [M] and counts [M][M].  Options: NULL takes the defaults.
 *   LVBA_ERR_ARG: a null required pointer, a non-finite pose or intrinsic, an option outside its range below, grid_x > W - 1 or
 *   grid_y > H - 1, capacity < 0, capacity > 0 with pairs NULL.  LVBA_ERR_UNSUPPORTED: M > 8192 (the count matrix would pass
 *   256 MB).  M = 0 and M = 1 give *count = 0.  A refused call writes nothing.  The defaults were chosen on synthetic scenes only.
 *   lvba_version() is unchanged; a client detects these calls by looking lvba_covis_pairs up. */
typedef struct lvba_covis_opts {
    int32_t grid_x, grid_y;      /* 1 .. 64 each, <= W - 1 / H - 1 (defaults 16, 12) */
    int32_t search_radius;       /* 0 .. 16 (default 4) */
    int32_t occlusion;           /* 0 or 1 (default 1) */
    int32_t both_ways;           /* 0 or 1 (default 0) */
    int32_t max_per_image;       /* 0 = no cap, else 1 .. 1024 (default 0) */
    int32_t min_shared;          /* samples, >= 0 (default 8) */
    int32_t reserved;
    double min_overlap;          /* finite, 0 .. 1 (default 0.1) */
    double occlusion_rel, occlusion_abs;  /* finite, >= 0 (defaults 0.05, 0.1 m) */
} lvba_covis_opts;               /* 56 bytes */
void    lvba_covis_default_opts(lvba_covis_opts *o);
int32_t lvba_covis_samples(lvba_depth_t depth, const double *Rcw, const double *tcw, const double intr[8],
                           const lvba_covis_opts *o, double *world /* [M][G][3], NaN = none */);
int32_t lvba_covis_counts(lvba_depth_t depth, const double *Rcw, const double *tcw, const double intr[8],
                          const lvba_covis_opts *o, int32_t *n_points /* [M] */, int32_t *counts /* [M][M] */);
int32_t lvba_covis_pairs(lvba_depth_t depth, const double *Rcw, const double *tcw, const double intr[8],
                         const lvba_covis_opts *o, int64_t capacity, int32_t *pairs, double *score, int32_t *shared,
                         int64_t *count);

/* ---- feature tracks on the device: match-graph components in BFS order (opt-in)
 *   The adjacency and BFS part of BuildTracksAndFuse3D (src/lvba_system.cpp:932-1014): what feeds lvba_fuse_tracks.  Every output
 *   is a discrete structure with one right answer; the host mirror (pipeline.match_graph / match_components / bfs_order, pinned to
 *   the reference by the tests) is the specification.
 *   Nodes.  Images 0 .. M - 1, image i has n_i = kp_off[i + 1] - kp_off[i] key points; key point k of image i is node
 *     v = kp_off[i] + k: node order is scan order (image, key point).
 *   Pairs and matches.  pairs [n_pairs][2] = (a, b) in any order and either orientation; the matches of pair p are the rows
 *     match_off[p] .. match_off[p + 1] of matches [][2] = (r in a, c in b) -- the arrays lvba_match_pairs writes.  A pair with
 *     a > b is read with its columns swapped, as (lo, hi).  The pairs are ranked by a STABLE sort on (lo, hi): a pair listed twice
 *     keeps the caller's order.
 *   Edge sequence.  The sequence number of an edge is (rank of its pair, position inside the pair).  A match with an index < 0 or
 *     >= the image's key point count is skipped and counted in n_skipped.
 *   Adjacency.  The neighbours of a node are listed by ascending edge sequence, duplicates kept.
 *   Components.  Connected components over the nodes with at least one edge.  A component QUALIFIES iff it has >= obser_thr members
 *     and they lie in >= obser_thr distinct images.  Qualifying components are numbered by ascending smallest member; members(c)
 *     are its nodes in ascending order.
 *   Order.  order(c, attempt) is the FIFO BFS from members(c)[attempt]: a popped node's neighbours are visited in adjacency order,
 *     a node is appended at its first visit.  attempt = 0 is the reference's first try; a component the fusion drops is met again
 *     at its next member (:1197, :1203), i.e. attempt + 1.
 *   lvba_trackgraph_create uploads once, builds everything up to the component table and leaves the adjacency and the tables
 *   resident.  keypoints_uv [kp_off[M]][2] may be NULL (then no call may ask for obs_uv).  info may be NULL.
 *   lvba_trackgraph_components: comp_off [n_components + 1], (mem_img, mem_kp) [n_observations] = members(c) of every component,
 *   comp_images [n_components] (may be NULL) the distinct images of each.
 *   lvba_trackgraph_orders: the orders of the n components comp[] (strictly ascending; NULL: all of them, n = n_components) for one
 *   attempt, obs_off [n + 1] and (obs_img, obs_kp, obs_uv) sized by the caller from comp_off; obs_uv may be NULL.  May be called any
 *   number of times; calls on one handle must not overlap (the visited marks are the handle's).
 *   The component labels are found with atomicMin; their fixed point is unique (the smallest node of each component), so every
 *   output is the same bytes on every call -- cc_rounds alone, the number of label rounds, is a diagnostic that may differ.
 *   LVBA_ERR_ARG, with nothing written: a null required pointer, a negative count, kp_off or match_off that does not start at 0 or
 *   decreases, a pair index outside the images, a == b, obser_thr < 1, comp not strictly ascending or out of range, attempt < 0 or
 *   >= the size of a requested component, obs_uv of a graph created without key points.  LVBA_ERR_UNSUPPORTED: kp_off[M] >= 2^31 or
 *   match_off[n_pairs] >= 2^30 (node and half-edge ids are 32 bits; checked before anything is read or allocated).
 *   LVBA_ERR_STATE: the label rounds passed their cap of 64, or a walk did not end at its component's size (neither can happen
 *   unless the library is wrong; every device loop is bounded, so such a fault is a code, not a hang).  M = 0, no pairs, no matches or
 *   all matches skipped give a valid empty graph.  lvba_version() is unchanged; a client detects these calls by looking
 *   lvba_trackgraph_create up. */
typedef struct lvba_trackgraph_s *lvba_trackgraph_t;
typedef struct lvba_trackgraph_info {
    int64_t n_nodes;          /* nodes with at least one edge */
    int64_t n_edges, n_skipped;
    int64_t n_components_all; /* before the two size checks */
    int64_t n_components, n_observations;   /* qualifying, and the sum of their sizes */
    int64_t largest_component;              /* the size of the largest qualifying one */
    int32_t cc_rounds, reserved;
} lvba_trackgraph_info;          /* 64 bytes */
int32_t lvba_trackgraph_create(int32_t device, int32_t n_images, const int64_t *kp_off /* [M+1], from 0 */,
                               const float *keypoints_uv /* [kp_off[M]][2], may be NULL */,
                               int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                               int32_t obser_thr, lvba_trackgraph_t *out, lvba_trackgraph_info *info);
int32_t lvba_trackgraph_components(lvba_trackgraph_t g, int64_t *comp_off /* [n_components+1] */,
                                   int32_t *mem_img, int32_t *mem_kp /* [n_observations] */,
                                   int32_t *comp_images /* [n_components] distinct images, may be NULL */);
int32_t lvba_trackgraph_orders(lvba_trackgraph_t g, int64_t n, const int64_t *comp /* strictly ascending; NULL: all, n = n_components */,
                               int32_t attempt, int64_t *obs_off /* [n+1] */, int32_t *obs_img, int32_t *obs_kp,
                               float *obs_uv /* [.][2]; may be NULL; needs keypoints_uv */);
int32_t lvba_trackgraph_destroy(lvba_trackgraph_t g);

/* ---- two-view verification of putative matches: batched RANSAC (opt-in)
 *   The reference reads geometrically verified inlier matches from its COLMAP database (loadFromColmapDB); matches that come from
 *   lvba_match_pairs, or from anywhere else, have seen no geometry, or only the geometry of poses that may themselves be in doubt.
 *   This stage estimates an essential matrix per image pair from the matches alone (method 0) or from the matches and the relative
 *   ROTATION of the two cameras (method 1) and keeps the matches that agree with it.  The rule below is this project's own
 *   definition, restated in numpy in tests/verify_oracle.py; it is NOT pinned against COLMAP's estimators.
 *   Inputs.  Keypoints (u, v) are fp32 pixels, undistorted once on the device (trk_undistort with intr; x^ = (x, y, 1), NaN where it
 *     fails).  pairs [P][2] = (a, b), a != b, either orientation; the matches of pair p are rows match_off[p] .. match_off[p + 1] of
 *     matches [][2] = (keypoint of a, keypoint of b), the arrays lvba_match_pairs writes.  "lo" is the image with the smaller index,
 *     "hi" the other; E maps lo to hi, x^_hi^T E x^_lo = 0 (the guided matcher's convention).  A pair given as (hi, lo) gives the
 *     same E and the same inliers as (lo, hi), in the caller's column order.
 *   Inlier test.  Match i is an inlier of E iff the guided matcher's gate passes it: with l = E x^_lo, l' = E^T x^_hi and
 *     tau = 2 max_error_px / (fx + fy),  (x^_hi . l)^2 <= tau^2 (l0^2 + l1^2 + l'0^2 + l'1^2)  (match_line_lo, match_norm_hi,
 *     match_gate of csrc/match_device.h, evaluated without contraction).  A NaN point is never an inlier.
 *   Sampling.  Hypothesis h of the pair draws k distinct positions of the pair's match list.  Draw j is r_j = mix(key + G (j + 1)),
 *     key = mix(mix(mix(seed + G) ^ (lo << 32 | hi)) + G (h + 1)), mix = splitmix64's finaliser, G = 0x9E3779B97F4A7C15: a
 *     function of (seed, lo, hi, h, j) alone -- not of the pair's place in the call, the grid or the lane.  r is mapped onto [0, n)
 *     as the high half of r n.  Draw j is taken from [0, m - j) and stepped past the positions already chosen, in ascending order
 *     (a partial Fisher-Yates shuffle without its array).  A pair verified alone, in a batch, or in a batch in another order
 *     gives the same bytes.
 *   Method 0, LVBA_VERIFY_EIGHT_POINT (pose-free), k = 8.  Row i of the 8 x 9 system is x^_hi (x) x^_lo.  vec(E) is its null vector
 *     by Gauss-Jordan elimination with full pivoting in the order of operations of verify_eight_solve (csrc/verify_device.h): the
 *     pivot of step s is the largest |entry| of rows s.. and columns s.., the lowest (row, column) of a tie; row exchange, column
 *     exchange, the pivot row divided, every other row reduced.  E is scaled to unit Frobenius norm.  The hypothesis is INVALID
 *     if a pivot is <= VERIFY_PIVOT_REL (1e-10) times the system's largest entry (repeated matches, collinear or otherwise
 *     degenerate samples) or a sample point is NaN.  Hypotheses are not projected onto the essential manifold; the test above
 *     does not need it.  THIS SOLVER IS DEGENERATE ON A SCENE THAT IS ONE PLANE (the system has rank 6 there): use method 1.
 *   Method 1, LVBA_VERIFY_KNOWN_ROTATION (rotation-aided), k = 2, needs Rcw at lvba_verify_create.  R = R_hi R_lo^T is trusted
 *     (odometry and the IMU give relative rotation to a fraction of a degree), the translation is not (position is what drifts).
 *     c_i = x^_hi,i x (R x^_lo,i), t = c_1 x c_2, E = [t]x R scaled to unit norm; INVALID if |t|^2 <= VERIFY_T_REL2 (1e-20)
 *     |c_1|^2 |c_2|^2 or a sample point is NaN.  Not degenerate on planes, and two-point samples survive low inlier ratios.
 *   Choice.  A hypothesis scores its inlier count, an invalid one -1; the highest count wins, the lowest h of a tie.  Integers
 *     only.  hypotheses (default 1024) is fixed, there is no early exit: 1 - (1 - w^k)^H at H = 1024 is 0.98 for method 0 at an
 *     inlier ratio w = 0.5 and above 0.9999 from w = 0.6; for method 1 it is above 0.9999 already at w = 0.2.
 *   Local refinement (refine_rounds, default 2, 0 = off).  The winner is refitted over its inliers and the refit kept only if its
 *     count is strictly larger.  Method 0: the eigenvector of the smallest eigenvalue of N = sum a a^T (9 x 9, cyclic Jacobi, 12
 *     sweeps), projected onto the essential manifold through the eigenvectors of E^T E.  Method 1: t = the smallest eigenvector
 *     of sum c c^T.  The refits go through libm; they are held to a measured tolerance, not to the bit.
 *   Status per pair.  LVBA_VERIFY_OK; LVBA_VERIFY_TOO_FEW_MATCHES: m < max(k, min_inliers) (no hypothesis is formed, E = 0,
 *     best_h = -1); LVBA_VERIFY_NO_MODEL: every hypothesis invalid (E = 0, best_h = -1); LVBA_VERIFY_TOO_FEW_INLIERS: count <
 *     min_inliers (default 15, the bound COLMAP's two-view geometry uses by default; E, count and best_h are reported).  A pair
 *     that is not OK contributes no inlier matches; it keeps its place in every output array.
 *   lvba_verify_create: kp_off [n_images + 1] from 0, keypoints_uv [kp_off[n_images]][2], intr = (fx, fy, cx, cy, k1, k2, p1, p2),
 *   Rcw [n_images][9] (T_cam<-world rotations) or NULL (method 0 only).
 *   lvba_verify_pairs: all pairs of the call in one grid.  inliers [capacity][2] in (pair, original order), inlier_off [n_pairs + 1]
 *   the first inlier of each pair and, last, the true number of inliers -- also where it exceeds capacity; only the first
 *   `capacity` are written (the convention of lvba_match_pairs).  E [n_pairs][9], status, n_inliers, best_h [n_pairs].
 *   lvba_verify_hypotheses: the diagnostic call, one pair: E [hypotheses][9] and count [hypotheses] of every hypothesis before the
 *   choice, without refinement (invalid: E = 0, count = -1).  It reads method, hypotheses, max_error_px and seed only.
 *   lvba_verify_score: mask [n_matches] (0 / 1) of the inlier test under a given E (lo -> hi).
 *   LVBA_ERR_ARG: method 1 on a handle without rotations, a == b or an image out of range, a match index outside its image,
 *   hypotheses < 1, a null required pointer or an option out of range.  lvba_version() is unchanged; a client detects these calls
 *   by looking lvba_verify_create up.
 *
 *   The homography model and the E-or-H choice (opt-in; lvba_verify_pairs_model, lvba_verify_hypotheses_homography,
 *   lvba_verify_score_homography; the calls above are untouched and lvba_verify_opts::method takes 0 and 1 only).  On a scene that
 *   is one plane a family of essential matrices takes every true match in and RANSAC picks the member that scoops up the most wrong
 *   ones; a point-to-line test cannot tell.  The model for a plane is point-to-point.  This rule, too, is the project's own
 *   (tests/verify_h_oracle.py) and is NOT pinned against COLMAP.
 *   Model.  H maps lo to hi in undistorted normalised coordinates: p = H x^_lo ~ x^_hi.
 *   Sample and system.  k = 4, the sampler and key above.  Sample point i fills rows 2 i and 2 i + 1 of an 8 x 9 system:
 *     (x_l, y_l, 1, 0, 0, 0, -x_h x_l, -x_h y_l, -x_h) and (0, 0, 0, x_l, y_l, 1, -y_h x_l, -y_h y_l, -y_h).
 *   Solve.  vec(H) is the null vector by verify_eight_solve as it stands: the pivot order, VERIFY_PIVOT_REL and the unit Frobenius
 *     norm of method 0.  Three collinear sample points lose a pivot: INVALID, as is a NaN sample point.
 *   Sign.  H is negated if p2 < 0 at the first sample point; p2 == 0 there is INVALID.
 *   Inverse direction.  G = adj(H), negated if det H < 0: a positive multiple of H^-1.  det H = (H0 G0 + H1 G3) + H2 G6 (the first
 *     row of H on the first column of adj(H)) must be finite and non-zero, else INVALID.  +, -, *, / and sqrt only, each sum in
 *     the order of verify_homography_inverse: a hypothesis is the same bits under g++, numpy and gfx950.
 *   Inlier test.  tau as above.  Match i is an inlier iff (p0 - x_h p2)^2 + (p1 - y_h p2)^2 <= tau^2 p2^2 and p2 > 0 with
 *     p = H x^_lo, and (q0 - x_l q2)^2 + (q1 - y_l q2)^2 <= tau^2 q2^2 and q2 > 0 with q = G x^_hi.  A NaN point fails.
 *   Choice, status.  As above, with k = 4.
 *   Local refinement.  N = sum (r1 r1^T + r2 r2^T) over the inliers, r1 and r2 the match's two rows; the eigenvector of its
 *     smallest eigenvalue by the same Jacobi (the lowest column of a tie), unit norm, negated if its Frobenius inner product with
 *     the current H is negative; no projection; G from it as above (no G: no refit).  Kept only if strictly more inliers.
 *   E-or-H choice, LVBA_VERIFY_MODEL_AUTO.  Each pair is run to completion under E (o->method, 0 or 1) and under H.  The pair is
 *     HOMOGRAPHY iff the H run is OK and either the E run is not OK or (double)n_H >= planar_ratio * (double)n_E; otherwise
 *     ESSENTIAL.  Every output of the pair is the chosen run's, byte for byte.  planar_ratio: finite and > 0;
 *     LVBA_VERIFY_PLANAR_RATIO (0.8, the value of COLMAP's max_H_inlier_ratio) sits in the middle of the gap the fixtures show
 *     between a plane (>= 0.89) and general position (<= 0.28).
 *   lvba_verify_pairs_model: lvba_verify_pairs with `model`; M [n_pairs][9] is E or H by kind [n_pairs] (LVBA_VERIFY_MODEL_ESSENTIAL
 *   or _HOMOGRAPHY).  n_inliers_E, n_inliers_H [n_pairs], either may be NULL: the inlier count of that model's run of the pair, -1
 *   where the model was not run.  LVBA_VERIFY_MODEL_ESSENTIAL gives the bytes of lvba_verify_pairs.  Under _HOMOGRAPHY o->method is
 *   not read.  AUTO adds no kernel: two runs, the decision on the host.
 *   lvba_verify_hypotheses_homography: the diagnostic call, H [hypotheses][9] and count; reads hypotheses, max_error_px, seed.
 *   lvba_verify_score_homography: the mask of the inlier test under a given H (lo -> hi); all 0 where det H is 0 or not finite.
 *   LVBA_ERR_ARG: an unknown model, a planar_ratio that is not finite or not > 0, and the refusals above.  lvba_version() is
 *   unchanged; a client detects these calls by looking lvba_verify_pairs_model up.
 *   Not built: several planes per pair (peeling the inliers and repeating), a pose from H, a path in lvba_adapter.hpp. */
#define LVBA_VERIFY_EIGHT_POINT 0
#define LVBA_VERIFY_KNOWN_ROTATION 1
#define LVBA_VERIFY_OK 0
#define LVBA_VERIFY_TOO_FEW_MATCHES 1
#define LVBA_VERIFY_NO_MODEL 2
#define LVBA_VERIFY_TOO_FEW_INLIERS 3
typedef struct lvba_verify_s *lvba_verify_t;
typedef struct lvba_verify_opts {
    int32_t method;        /* LVBA_VERIFY_EIGHT_POINT (default) or LVBA_VERIFY_KNOWN_ROTATION */
    int32_t hypotheses;    /* 1024 */
    int32_t refine_rounds; /* 2; 0 = off */
    int32_t min_inliers;   /* 15 */
    double max_error_px;   /* 4.0, the guided matcher's max_epipolar_px */
    uint64_t seed;         /* 0 */
} lvba_verify_opts;        /* 32 bytes */
void    lvba_verify_default_opts(lvba_verify_opts *o);
int32_t lvba_verify_create(int32_t device, int32_t n_images, const int64_t *kp_off, const float *keypoints_uv, const double *intr,
                           const double *Rcw_or_null, lvba_verify_t *out);
int32_t lvba_verify_destroy(lvba_verify_t v);
int32_t lvba_verify_pairs(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                          const lvba_verify_opts *o, int64_t capacity, int64_t *inlier_off, int32_t *inliers, double *E,
                          int32_t *status, int32_t *n_inliers, int32_t *best_h);
int32_t lvba_verify_hypotheses(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches,
                               const lvba_verify_opts *o, double *E, int32_t *count);
int32_t lvba_verify_score(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const double *E,
                          double max_error_px, uint8_t *mask);
#define LVBA_VERIFY_MODEL_ESSENTIAL 0
#define LVBA_VERIFY_MODEL_HOMOGRAPHY 1
#define LVBA_VERIFY_MODEL_AUTO 2
#define LVBA_VERIFY_PLANAR_RATIO 0.8
int32_t lvba_verify_pairs_model(lvba_verify_t v, int64_t n_pairs, const int32_t *pairs, const int64_t *match_off, const int32_t *matches,
                                const lvba_verify_opts *o, int32_t model, double planar_ratio, int64_t capacity, int64_t *inlier_off,
                                int32_t *inliers, double *M, int32_t *kind, int32_t *status, int32_t *n_inliers, int32_t *best_h,
                                int32_t *n_inliers_E_or_null, int32_t *n_inliers_H_or_null);
int32_t lvba_verify_hypotheses_homography(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches,
                                          const lvba_verify_opts *o, double *Hm, int32_t *count);
int32_t lvba_verify_score_homography(lvba_verify_t v, int32_t a, int32_t b, int64_t n_matches, const int32_t *matches, const double *Hm,
                                     double max_error_px, uint8_t *mask);

/* ---- SIFT key points and descriptors of a batch of images (opt-in)
 *   The reference extracts its features with SiftGPU, "-fo -1 -loweo -w 3 -t 0.01 -e 12" (extractAndMatchFeaturesGPU,
 *   src/lvba_system.cpp:687-778).  The rule below is this project's own reading of Lowe 2004 under those five parameters; it is NOT
 *   pinned against SiftGPU, whose key points it will not reproduce one for one.  A numpy oracle restates it (tests/sift_oracle.py).
 *   The descriptors have the form lvba_match_create takes: uint8 [n][128], a unit vector times 512.
 *   Every product and sum below is evaluated as written, left to right inside its brackets, without fused multiply-add.
 *   Grey (fp32).  From uint8 B, G, R:  g = ((0.299f R + 0.587f G) + 0.114f B) / 255.0f;  from a grey byte v:  g = v / 255.0f.
 *   Base image (fp32).  first_octave = -1 doubles the image, first along the rows,
 *       H(y, 2 x) = g(y, x),   H(y, 2 x + 1) = 0.5f (g(y, x) + g(y, min(x + 1, w - 1))),
 *     then along the columns,  B(2 y, X) = H(y, X),   B(2 y + 1, X) = 0.5f (H(y, X) + H(min(y + 1, h - 1), X));
 *     its assumed blur is 1.0 (0.5 before the doubling).  first_octave = 0 takes B = g with assumed blur 0.5.
 *     Level 0 of the first octave is B blurred with sigma = sqrt(sigma0^2 - assumed^2).
 *   Pyramid (fp32).  S = n_intervals; an octave has the Gaussian levels 0 .. S + 2, level l from level l - 1 by a blur with
 *       sigma_inc(l) = sigma0 2^((l - 1) / S) sqrt(2^(2 / S) - 1).
 *     A blur is separable, rows first, then columns.  Radius r = ceil(4 sigma); taps t[k], k = -r .. r: exp(-k^2 / (2 sigma^2)) in
 *     fp64 on the host, divided by their sum (ascending k), rounded to fp32 -- computed once per call (lvba_sift_blur_taps hands
 *     them out; level 0 is the base blur).  out(x) = t[-r] in(c(x - r)), then + t[k] in(c(x + k)) for k = -r + 1 .. r in this order,
 *     every product and sum rounded to fp32; c clamps an index into the image, and r may exceed the image.
 *     Level 0 of the next octave is level S at every second pixel, (2 x, 2 y), with w' = w / 2, h' = h / 2 in integer division; the
 *     octaves o = first_octave, first_octave + 1, ... go on while min(w', h') >= 8.
 *   Extrema.  DoG level l = Gaussian level l + 1 minus level l in fp32, l = 0 .. S + 1.  The sample (l, y, x), 1 <= l <= S,
 *     1 <= x <= w - 2, 1 <= y <= h - 2, is a candidate iff  (double)|D| > (0.5 t) / S  and D is strictly greater than all of its 26
 *     neighbours or strictly less than all of them  (t = dog_threshold).
 *   Refinement (fp64 on the fp32 DoG values, only + - * /; csrc/sift_device.h, sift_refine, is the text).  At the sample:
 *       g = 0.5 (D(+1) - D(-1)) per axis;  H_aa = (D(+1) + D(-1)) - 2 D;  H_ab = 0.25 ((D(+a+b) - D(+a-b)) - (D(-a+b) - D(-a-b)))
 *       with the later axis of (x, y, l) as a;  the offset (ox, oy, ol) = -(adj(H) g) / det(H) by the explicit cofactors, the three
 *       products of a row summed left to right.  det = 0: dropped.
 *     While a component exceeds 0.5 in magnitude the sample moves by +-1 along every such axis, at most 5 moves; the key point is
 *     dropped when it leaves 1 <= x <= w - 2, 1 <= y <= h - 2, 1 <= l <= S, when an offset still exceeds 0.5 after the fifth move,
 *     when |D + 0.5 ((gx ox + gy oy) + gl ol)| < t / S, when Hxx Hyy - Hxy Hxy <= 0 or when
 *     (Hxx + Hyy)^2 / (Hxx Hyy - Hxy Hxy) >= (e + 1)^2 / e  (e = edge_threshold).
 *     sigma_o = sigma0 2^((l + ol) / S) with 2^z from sift_pow2 of sift_device.h (+ * / only, so host and device agree);
 *     x = (x_s + ox) 2^o, y = (y_s + oy) 2^o, sigma = sigma_o 2^o, rounded to float: input pixels, (0, 0) the centre of the first
 *     pixel.  Two candidates may end on the same sample; both are kept.
 *   Orientation (fp64 on the fp32 pixels of Gaussian level l of the octave -- the level nearest the refined scale, |ol| <= 0.5).
 *     R = floor(w_f 1.5 sigma_o + 0.5)  (w_f = orientation_window).  For j = -R .. R and inside that i = -R .. R with
 *     i i + j j <= R R and (x_s + i, y_s + j) in [1, w - 2] x [1, h - 2]:  gx = L(+1, 0) - L(-1, 0), gy = L(0, +1) - L(0, -1),
 *       weight = exp(-((i - ox)^2 + (j - oy)^2) / (2 (1.5 sigma_o)^2)),  a = atan2(gy, gx) (+ 2 pi if negative),
 *       bin = min(35, (int)(a (36 / 2 pi))),  hist[bin] += sqrt(gx gx + gy gy) weight   -- every bin summed in this sample order.
 *     Twice: hist[k] = ((hist[k - 1] + hist[k]) + hist[k + 1]) / 3 around the circle.  A bin strictly above both neighbours and
 *     >= 0.8 max is a peak;  theta = ((k + 0.5) + (0.5 (h[k-1] - h[k+1])) / ((h[k-1] - 2 h[k]) + h[k+1])) (2 pi / 36), wrapped into
 *     [0, 2 pi), rounded to float.  At most max_orientations are kept, the larger peak first (a tie: the lower bin); a key point
 *     without a peak is dropped.  The angle runs from +x towards +y (y points down the image).
 *   Descriptor (fp64; the float theta widened again).  Bin width 3 sigma_o, 4 x 4 cells of 8 directions, window radius
 *     R = floor(((3 sigma_o) sqrt(2)) 2.5 + 0.5).  For j, i = -R .. R as above, with dx = i - ox, dy = j - oy:
 *       rx = (cos dx + sin dy) / (3 sigma_o),  ry = (cos dy - sin dx) / (3 sigma_o),  cb = rx + 1.5,  rb = ry + 1.5,
 *       used iff -1 < rb < 4 and -1 < cb < 4;  a = atan2(gy, gx) - theta wrapped into [0, 2 pi),  ob = a (8 / 2 pi),
 *       v = sqrt(gx gx + gy gy) exp(-(rx rx + ry ry) / 8)   (a Gaussian window of two cells),
 *       shared trilinearly: ((v w_r) w_c) w_o to the cells floor(rb), floor(rb) + 1 (inside 0 .. 3), likewise the columns, and the
 *       directions floor(ob), floor(ob) + 1 modulo 8; every bin summed in this sample order.  Byte (4 r + c) 8 + o.
 *     Then: divided by the L2 norm (sum of squares in byte order), clamped at 0.2, divided by the norm again,
 *       byte = min(255, floor(512 v + 0.5)).
 *   Output.  Per image in the canonical order: (octave, level and y, x of the sample the candidate was FOUND at, orientation rank).
 *     With more than max_features features an image keeps the max_features of largest float sigma (a tie: the earlier in the
 *     canonical order), still in canonical order.  count[i] is the number before that cap.  feat_off [n_images + 1] are the true
 *     offsets of the kept features, also where they exceed capacity; only the first `capacity` rows of keypoints [.][4] =
 *     (x, y, sigma, theta) and descriptors [.][128] are written.  Images: uint8 [n_images][height][width][channels], channels 3
 *     (B, G, R) or 1, all of one size.  chunk_images images share a pyramid on the device at a time (0: as many as half of the
 *     free memory holds, at most 64).  No floating-point atomics and no atomics at all: a pair of calls, a batch, a batch reversed
 *     and any chunk size give the same bytes per image.
 *   lvba_sift_blur_taps (host only, touches no device): taps [2 r + 1] (room for 65) and r of level 0 .. S + 2.
 *   lvba_sift_tile_width (host only): the pixels of a row one workgroup of the blur covers -- where a test puts its widths.
 *   lvba_sift_profile (host only): ms [6] of the calling thread's last lvba_sift_extract by the host's clock -- pyramid (upload, base
 *     image, blurs), detection (DoG, flags, scan, refinement), orientation, descriptor (with the download), assembly on the host,
 *     the whole call.
 *   lvba_sift_pyramid: a diagnostic; gauss [S + 3][h_o][w_o] and dog [S + 2][h_o][w_o] of one image's octave o.
 *   lvba_sift_candidates: a diagnostic; the refined key points of one image before the orientation: xys [capacity][3] =
 *     (x, y, sigma), where [capacity][2] = (octave, level of the sample the fit ended on), *count the true number.
 *   LVBA_ERR_ARG: a null required pointer, a negative count, width or height outside 8 .. 16384, channels not 1 or 3, an octave
 *   the image does not have, an option outside the range noted below, or a blur radius above 32.  A refused call writes nothing,
 *   and these refusals come before a device is touched.  lvba_version() is unchanged; a client detects these calls by looking
 *   lvba_sift_extract up. */
typedef struct lvba_sift_opts {
    int32_t first_octave;       /* -1 (default) or 0 */
    int32_t n_intervals;        /* S, 2 .. 5 (default 3) */
    double sigma0;              /* in [1.1, 4] (default 1.6) */
    double dog_threshold;       /* t, in (0, 1] (default 0.01) */
    double edge_threshold;      /* e, in [1, 1000] (default 12) */
    double orientation_window;  /* w_f, in [0.5, 6] (default 3) */
    int32_t max_orientations;   /* 1 .. 4 (default 2) */
    int32_t max_features;       /* >= 1 (default 8192) */
    int32_t chunk_images;       /* >= 0 (default 0: from the free memory) */
    int32_t reserved;           /* 0 */
} lvba_sift_opts;               /* 56 bytes */
void    lvba_sift_default_opts(lvba_sift_opts *o);
int32_t lvba_sift_tile_width(void);
int32_t lvba_sift_blur_taps(const lvba_sift_opts *o, int32_t level, float *taps, int32_t *radius);
int32_t lvba_sift_extract(int32_t device, int32_t n_images, int32_t width, int32_t height, int32_t channels, const uint8_t *images,
                          const lvba_sift_opts *o, int64_t capacity, int64_t *feat_off, float *keypoints, uint8_t *descriptors,
                          int64_t *count);
int32_t lvba_sift_profile(double *ms);
int32_t lvba_sift_pyramid(int32_t device, int32_t width, int32_t height, int32_t channels, const uint8_t *image,
                          const lvba_sift_opts *o, int32_t octave, float *gauss, float *dog);
int32_t lvba_sift_candidates(int32_t device, int32_t width, int32_t height, int32_t channels, const uint8_t *image,
                             const lvba_sift_opts *o, int64_t capacity, float *xys, int32_t *where, int64_t *count);

/* ---- Moving objects in the LiDAR map, by range-image visibility ------------------------------------------
 *   Every scan is a record of free space along its rays.  A point of frame f is not part of the static scene when some other
 *   frames measured a clearly longer range in the point's direction and in all neighbouring directions: they saw through it.
 *   This is the visibility test of Removert (Kim & Kim, IROS 2020), stated here as this library's own rule.  Everything is fp64 on
 *   the fp32 points promoted once, every expression rounded as written (no fused multiply-add).
 *   Frames [frame_begin, frame_begin + n_frames) of scans at scan_poses [n_frames][12] (R row-major | t, T_world<-body, relative
 *   to frame_begin as for the map quality); P = their number of points, in cloud order (frames in order, points in scan order).
 *   Cell of a body-frame point (x, y, z) in a range image of n_rows x n_cols:
 *     rho = sqrt(x x + y y),  r = sqrt((x x + y y) + z z);  no cell unless r is finite, min_range <= r < max_range and rho > 0;
 *     col = (int)floor((atan2(y, x) + pi) n_cols / (2 pi)), at most n_cols - 1;
 *     e = atan2(z, rho);  no cell unless el_min <= e < el_max;
 *     row = (int)floor((e - el_min) n_rows / (el_max - el_min)), at most n_rows - 1.
 *   Range image of frame g:  I_g[row][col] = the smallest (float)r of the frame's points with that cell, +inf without one.
 *   Dilated image:  M_g[row][col] = the smallest I_g over rows row - halo .. row + halo (those outside the image skipped) and
 *     columns col - halo .. col + halo (modulo n_cols).  A neighbouring direction that hits something nearer vetoes a
 *     see-through: grazing floor and wall points stay static at this angular resolution.
 *   Votes of point p of frame f:  w = R_f p + t_f (each row summed from left to right, kept in double).  For every frame g != f
 *     of the range with |g - f| <= window (window <= 0: every frame):  d = w - t_g,
 *     q_j = (R_g[0][j] d_0 + R_g[1][j] d_1) + R_g[2][j] d_2;  the cell of q and r_q by the rule above -- no cell, no evidence;
 *     m = M_g[cell] -- +inf, no evidence;  tol = abs_tol + rel_tol r_q;
 *     (double)m > r_q + tol: a FREE vote (g saw through the point);  else (double)m >= r_q - tol: a SUPPORT vote;  else the
 *     point is occluded in g: no evidence.  A non-finite point has no cell in its own image and collects no votes.
 *   Label:  1 (dynamic) iff n_free >= min_free and (double)n_free >= free_ratio (double)(n_free + n_support);  else 0.
 *   The defaults below are this library's choice; they are NOT tuned on real data.
 *   Outputs, each may be NULL: label [P] uint8, n_free [P], n_support [P].  Summary: n_judged = the points with at least one vote;
 *   ms = device time of the images, the dilation, the votes (with the labels), and the host's time of the download.
 *   The images of batch_frames frames are on the device at a time (0: as many as the free memory holds); votes are integer
 *   counts, so the outputs do not depend on the batching, and two calls give the same bytes.  No floating-point atomics.
 *   Options: NULL takes the defaults.
 *   LVBA_ERR_ARG: a null scans, scan_poses or summary pointer; a frame range outside the scans or n_frames < 1; a non-finite pose;
 *   n_rows outside 1 .. 1024, n_cols outside 1 .. 4096, halo outside 0 .. 3; el_min >= el_max or either outside [-pi/2, pi/2];
 *   min_range not in [0, max_range); a negative or non-finite tolerance; min_free < 1; free_ratio outside (0, 1];
 *   batch_frames < 0.  LVBA_ERR_NOMEM: the per-point counters and the images of one frame (or of batch_frames > 0 frames) do not
 *   fit into the free device memory.
 *   lvba_scans_select: a new scan set on the same device with the same number of frames, each frame keeping its points with
 *   keep != 0 in scan order (keep: host memory, one byte per point of the WHOLE set in cloud order; a frame may come out empty;
 *   the compaction runs on the device).  The result is a scan set like any other and is destroyed like any other.
 *   LVBA_ERR_ARG: a null scans or out pointer, a null mask for a set with points, 2^32 - 1 points or more.
 *   lvba_version() is unchanged; a client detects these calls by looking lvba_dynamic_labels up. */
typedef struct lvba_dynamic_opts {
    int32_t n_rows, n_cols;      /* the range image: 240 x 720 (0.5 degrees a cell) */
    int32_t halo;                /* 0 .. 3 (default 1) */
    int32_t window;              /* frames on either side that vote (default 20; <= 0: all) */
    int32_t min_free;            /* >= 1 (default 3) */
    int32_t batch_frames;        /* >= 0 (default 0: from the free memory) */
    double el_min, el_max;       /* elevation range in radians (default -pi/3, +pi/3) */
    double min_range, max_range; /* metres (default 0.5, 80) */
    double abs_tol, rel_tol;     /* tol = abs_tol + rel_tol r (default 0.2 m, 0.02) */
    double free_ratio;           /* in (0, 1] (default 0.5) */
} lvba_dynamic_opts;             /* 80 bytes */
typedef struct lvba_dynamic_summary {
    int64_t n_points, n_judged, n_dynamic;
    double ms[4];
} lvba_dynamic_summary;          /* 56 bytes */
void    lvba_dynamic_default_opts(lvba_dynamic_opts *o);
int32_t lvba_dynamic_labels(lvba_scans_t scans, const double *scan_poses, int32_t frame_begin, int32_t n_frames,
                            const lvba_dynamic_opts *o, lvba_dynamic_summary *summary, uint8_t *label, int32_t *n_free,
                            int32_t *n_support);
int32_t lvba_scans_select(lvba_scans_t scans, const uint8_t *keep, lvba_scans_t *out);

/* ---- camera resectioning from 2-D to 3-D matches: batched P3P RANSAC (opt-in)
 *   Every camera pose of the pipeline is derived (the LiDAR trajectory interpolated at the image time, times the extrinsic).  A
 *   matched keypoint whose partner has a LiDAR depth return is a 2-D to 3-D correspondence (lvba_match_set_depth lifts such points,
 *   lvba_resect_lift does the same for a batch of images without a matcher); three of them give the absolute pose of an image, of
 *   the run or foreign to it.  The rule below is this project's own definition, restated in numpy in tests/resect_oracle.py; it is
 *   NOT pinned against COLMAP's absolute-pose estimator.  fp64 throughout, every sum left to right, no contraction.
 *   Job.  One image: id (int32 >= 0, distinct within a call), m correspondences = rows corr_off[j] .. corr_off[j + 1] of uv [][2]
 *     (fp32 pixels) and world [][3] (fp64), and the call's intrinsics intr = (fx, fy, cx, cy, k1, k2, p1, p2).  Pixels are
 *     undistorted once on the device (trk_undistort; (x, y), NaN where it fails).  A correspondence with a NaN (x, y) or a
 *     non-finite X is UNUSABLE: never an inlier, and a sample that draws it is invalid.
 *   Inlier test of (R, t) = T_cam<-world.  Xc = R X + t, each row ((r0 X0 + r1 X1) + r2 X2) + t;  a = fx (Xc_x - x Xc_z),
 *     b = fy (Xc_y - y Xc_z);  inlier iff Xc_z > 1e-12 and a a + b b <= (rho Xc_z)(rho Xc_z), rho = max_error_px; false for any NaN.
 *     The reprojection error in undistorted pixels, division-free, with the cheirality bound of projectCameraToPixel.
 *   Sampling.  Hypothesis h draws k = 4 distinct positions with the two-view verification's sampler (above), its key formed with
 *     lo = id, hi = -1: a function of (seed, id, h, draw) alone, and apart from every image pair's stream (a pair has hi >= 1).
 *   Minimal solver (resect_p3p of csrc/resect_device.h, whose comment gives every expression in order) on the first three draws.
 *     Unit bearings f_i = (x_i, y_i, 1) / |.|; the depths s_i satisfy s_i^2 + s_j^2 - 2 s_i s_j (f_i . f_j) = a_ij = |X_i - X_j|^2,
 *     s^T M_ij s = a_ij.  D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 are zero on the solution (Persson and Nordberg, Lambda
 *     twist, ECCV 2018).  INVALID: |(X1 - X2) x (X1 - X3)|^2 <= 1e-12 a12 a13 (degenerate triangle).  One real root g of the cubic
 *     det(D1 + g D2), made monic (leading coefficient 0: INVALID), by 16 Newton steps, all taken (a step with a zero derivative is
 *     left out): with disc = b^2 - 3 c > 0 and the stationary points t1 < t2 = (-b -+ sqrt(disc)) / 3, from t1 - sqrt(p(t1) /
 *     sqrt(disc)) where p(t1) > 0 and from t2 + sqrt(-p(t2) / sqrt(disc)) otherwise; disc <= 0: from -b / 3.  D0 = D1 + g D2 has
 *     rank 2: B = -adj(D0), i its largest diagonal entry (lowest of a tie; <= 1e-14 max|D0|^2: INVALID -- no pair of real planes),
 *     p = B[:, i] / sqrt(B_ii), N = D0 + [p]x has rank 1, and with (r, c) its entry of largest magnitude (row by row, lowest of a
 *     tie) the planes are row r and column c of N.  Per plane n, with k its largest |n_k|, two vectors u, v of the plane; s = al u
 *     + be v in D1 is A al^2 + 2 B al be + C be^2 = 0; B^2 - A C < 0: no solution of that plane; q = -(B + sign(B) sqrt(B^2 - A C)),
 *     (al, be) = (q, A) and (C, q).  Up to four depth triples, number 2 plane + root.  Scale: lam^2 = (a12 + a13 + a23) / (the
 *     three left sides at s, summed), signed so that s1 > 0.  Three Gauss-Newton steps on (s1, s2, s3) against the three equations.
 *     A depth that is not finite or not > 0: no solution.  R = Y X^-1 with X = [X1 - X2, X1 - X3, (X1 - X2) x (X1 - X3)] and Y the
 *     same of s_i f_i (inverse by cofactors), t = s1 f1 - R X1.  +, -, *, / and sqrt only: the same sample gives the same bits
 *     under g++, numpy and gfx950.  The hypothesis is the solution with the smallest squared undistorted-pixel error (fx (Xc_x /
 *     Xc_z - x))^2 + (fy (Xc_y / Xc_z - y))^2 on the FOURTH draw, which must lie in front (Xc_z > 1e-12); lowest number of a tie.
 *     No such solution: the hypothesis is INVALID and counts -1.  Not degenerate on planes.
 *   Choice.  The highest inlier count wins, the lowest h of a tie; integers only.  hypotheses (default 1024) is fixed, no early
 *     exit: 1 - (1 - w^4)^H at H = 1024 is 0.9998 at an inlier ratio w = 0.3 and 1 - 2e-29 at w = 0.5.
 *   Refinement (refine_rounds, default 2, 0 = off).  A round takes 4 Gauss-Newton steps on the six pose parameters over the
 *     inliers of the round's starting pose: residual (fx (Xc_x / Xc_z - x), fy (Xc_y / Xc_z - y)), left perturbation Xc <- Xc +
 *     om x Xc + up in the order (om, up), the 6 x 6 normal equations by Cholesky column after column, R <- (I + [om]x) R
 *     re-orthonormalised through a unit quaternion (sqrt only), t <- t + om x t + up.  Then it rescores; the refit is kept iff its
 *     count is not smaller than before, and a round that is not kept ends the refinement.  The sums are a tree on the device:
 *     the refit is held to a measured tolerance, not to the bit.
 *   Status per job.  LVBA_RESECT_OK; LVBA_RESECT_TOO_FEW_MATCHES: m < max(4, min_inliers) (no hypothesis, pose 0, best_h = -1);
 *     LVBA_RESECT_NO_MODEL: every hypothesis invalid; LVBA_RESECT_TOO_FEW_INLIERS: count < min_inliers (pose, count and best_h are
 *     reported).  A job that is not OK keeps its place in every output and contributes no inliers.  min_inliers defaults to 30,
 *     the bound COLMAP uses to register an image as this project remembers it -- its own rule, not pinned; max_error_px defaults
 *     to 8, the depth gate's max_reproj_px (the same quantity).
 *   lvba_resect_images: all jobs of the call in one grid.  Rcw [n_jobs][9], tcw [n_jobs][3], status, n_inliers, best_h [n_jobs],
 *     rmse_px [n_jobs] over the final inliers, information [n_jobs][36] = sum J^T J at the final pose over the final inliers in
 *     px^-2 (order (om, up)), inliers [capacity] = positions within the job in (job, original order), inlier_off [n_jobs + 1] with
 *     the capacity convention of lvba_verify_pairs.
 *   lvba_resect_hypotheses: the diagnostic call, one job: R [hypotheses][9], t [hypotheses][3], count [hypotheses] of every
 *     hypothesis before the choice (invalid: zeros and -1).  lvba_resect_score: mask [m] of the inlier test under a given pose.
 *   lvba_resect_lift: the keypoints uv of the depth set's images (rows kp_off[i] .. kp_off[i + 1] belong to image i) through
 *     their depth images into world [kp_off[n_images]][3] -- match_lift, as lvba_match_set_depth does it -- NaN rows where a
 *     keypoint has no point.
 *   LVBA_ERR_ARG (nothing written): a null required pointer, a negative or repeated id, corr_off that does not start at 0 or
 *   decreases, non-finite intrinsics or focal lengths <= 0, hypotheses < 1, refine_rounds < 0, min_inliers < 0, max_error_px not
 *   finite or <= 0, a depth set of another image count, non-finite poses at the lift.  lvba_version() is unchanged; a client
 *   detects these calls by looking lvba_resect_images up. */
#define LVBA_RESECT_OK 0
#define LVBA_RESECT_TOO_FEW_MATCHES 1
#define LVBA_RESECT_NO_MODEL 2
#define LVBA_RESECT_TOO_FEW_INLIERS 3
typedef struct lvba_resect_opts {
    int32_t hypotheses;    /* 1024 */
    int32_t refine_rounds; /* 2; 0 = off */
    int32_t min_inliers;   /* 30 */
    int32_t reserved;      /* 0 */
    double max_error_px;   /* 8.0, the depth gate's max_reproj_px */
    uint64_t seed;         /* 0 */
} lvba_resect_opts;        /* 32 bytes */
void    lvba_resect_default_opts(lvba_resect_opts *o);
int32_t lvba_resect_images(int32_t device, int32_t n_jobs, const int32_t *ids, const int64_t *corr_off, const float *uv,
                           const double *world, const double *intr, const lvba_resect_opts *o, int64_t capacity, int64_t *inlier_off,
                           int32_t *inliers, double *Rcw, double *tcw, int32_t *status, int32_t *n_inliers, int32_t *best_h,
                           double *rmse_px, double *information);
int32_t lvba_resect_hypotheses(int32_t device, int32_t id, int64_t n_corr, const float *uv, const double *world, const double *intr,
                               const lvba_resect_opts *o, double *R, double *t, int32_t *count);
int32_t lvba_resect_score(int32_t device, int64_t n_corr, const float *uv, const double *world, const double *intr, const double *Rcw,
                          const double *tcw, double max_error_px, uint8_t *mask);
int32_t lvba_resect_lift(lvba_depth_t depth, int32_t n_images, const int64_t *kp_off, const float *uv, const double *intr,
                         const double *Rcw, const double *tcw, double *world);

/* ---- LiDAR-camera extrinsic refinement from depth-lifted matches (opt-in)
 *   Every camera pose of the pipeline is the body pose at the image time times ONE configured transform T_cam<-imu = (Rci, tci).
 *   A match between images a and b whose keypoint in b has a LiDAR depth return constrains that transform through the body's motion
 *   between the two image times: the hand-eye equation A X = X B, with metric scale from the LiDAR.  These calls minimise the
 *   reprojection error of all such records over the six parameters of X by Gauss-Newton, hold the directions the trajectory leaves
 *   unobservable, and say which they are.  The rule below is this project's own definition, restated in numpy in
 *   tests/calib_oracle.py.  fp64 throughout, every sum left to right within a record, no contraction: a record's residual, Jacobian
 *   and weight are the same bits under g++, numpy and gfx950; the sums over the records are a tree on the device and are held to the
 *   summation bound.
 *   Record.  pair (int32, a row of the pair table), uv_a (fp32 pixel of the keypoint in the TARGET image a), Xb (fp64 [3]: the
 *     partner keypoint's lifted point in the camera frame of the SOURCE image b, at the pose it was lifted with).  Records arrive
 *     grouped by pair: all records of a pair in one run.
 *   Pair table.  img_a, img_b [n_pairs], a directed pair each.  Body poses: T_world<-imu [n_images][12] (R row-major, then P), the
 *     layout of image_poses.
 *   Once per call, on the device.  Per pair R_ab = Rwi_a^T Rwi_b, p_ab = Rwi_a^T (P_b - P_a) (T_imu_a<-imu_b); per record (x, y) =
 *     uv_a undistorted (trk_undistort, intr = (fx, fy, cx, cy, k1, k2, p1, p2)).  A record whose (x, y) is NaN or whose Xb is not
 *     finite is UNUSABLE: never counted.
 *   Residual at (R, t) = (Rci, tci).  q = R^T (Xb - t);  w = R_ab q + p_ab;  Xc = R w + t, every row ((m0 v0 + m1 v1) + m2 v2) +
 *     c;  iz = 1 / Xc_z, r = (fx (Xc_x iz - x), fy (Xc_y iz - y)) (the resection's refit form).  The record COUNTS iff Xc_z > 1e-12
 *     and, where max_error_px > 0, r0 r0 + r1 r1 <= max_error_px max_error_px -- at the extrinsic the iteration starts from, so
 *     the counted set may change from one iteration to the next.
 *   Jacobian under the resection's left perturbation (R <- (I + [om]x) R re-orthonormalised through a unit quaternion, t <- t +
 *     om x t + up, order (om, up)): with M = R R_ab R^T, dXc/dom = -[Xc]x + M [Xb]x and dXc/dup = I - M, each followed by the 2 x 3
 *     projection Jacobian.  I - M is why the translation needs rotation about two axes.  csrc/calib_device.h writes every
 *     expression in order (M is never formed: a Jacobian row is Xc x g + h x Xb, g - h with h = R (R_ab^T (R^T g))).
 *   Loss.  loss_eval of csrc/visual_loss.h on s = |r|^2 at scale loss_scale_px, kinds LVBA_LOSS_*: weight rho', cost rho / 2.
 *     Default Huber at 2 px: the value of the numpy prototype this stage started from, not tuned on recorded data.
 *   Sums.  H = sum rho' J^T J (21), g = sum rho' J^T r (6), cost = sum rho / 2, the count, sum |r|^2, sum rho'.
 *   Step.  H = V diag(lambda) V^T by cyclic Jacobi, eigenvalues ascending.  Direction k is HELD where not lambda_k > min_eig_ratio
 *     lambda_max (default 1e-6: between the 1.3e-3 of a trajectory that rotates about three axes and the 1e-15 of one that rotates
 *     about one, as the prototype saw them; not measured on recorded data).  The step is the Gauss-Newton step in the span of the
 *     free directions, d = -sum_free v_k (v_k . g) / lambda_k.  CONVERGED where |om| <= eps_rot and |up| <= eps_trans (defaults
 *     1e-10 rad, 1e-10 m); that step is not applied.  At most max_iterations (default 20) steps, then one more linearisation:
 *     whatever the status, n_used, rmse_px, cost, the eigen-decomposition and information are of the extrinsic returned.
 *   Status per job.  LVBA_CALIB_CONVERGED; LVBA_CALIB_MAX_ITERATIONS; LVBA_CALIB_TOO_FEW_RECORDS: fewer than min_records (default
 *     100) records count (no eigen-decomposition: zeros); LVBA_CALIB_DEGENERATE: lambda_max is not > 0 -- up to rounding: not above
 *     1e-20 n_used (fx^2 + fy^2), the square of the Jacobian's own rounding being all H holds where the body never moves --,
 *     every direction is held, or the step is not finite.  n_held (0 .. 6) is an output of its own, not a failure: a body that
 *     turns about one axis and moves only along it comes back CONVERGED with n_held = 2 (the rotation about that axis and the
 *     translation along it); a ground vehicle, which also moves across its axis, with n_held = 1 (the translation along it: the
 *     motion across ties the rotation down through the LiDAR's metric scale).
 *   Jobs.  n_jobs initial extrinsics over the SAME records (multi-start), iterated in lock-step.  What a job returns depends
 *     neither on what else is in the batch nor on its place in it.
 *   lvba_calib_extrinsic: per job Rci_out [9], tci_out [3], status, iterations (steps applied), n_used, rmse_px = sqrt(sum |r|^2 /
 *     n_used), cost, n_held, eigenvalues [6] ascending, eigenvectors [36] (row k the unit vector of eigenvalue k, order (om, up),
 *     camera frame), information [36] = H at the returned extrinsic, px^-2.
 *   lvba_calib_linearize: the diagnostic call, one evaluation per job at the given extrinsic and no step: H [n_jobs][36], g [6],
 *     cost, n_used, sum_sq = sum |r|^2.
 *   LVBA_ERR_ARG (nothing written): a null pointer, n_images < 1, n_jobs < 1, a negative count, a pair index outside the table,
 *   records not grouped by pair, an image index outside [0, n_images) or img_a == img_b, non-finite poses, intrinsics or initial
 *   extrinsic, focal lengths <= 0, max_iterations < 1 (or > 1000), a negative or NaN threshold, an unknown loss or a loss scale that
 *   is not > 0.  lvba_version() is unchanged; a client detects these calls by looking lvba_calib_extrinsic up. */
#define LVBA_CALIB_CONVERGED 0
#define LVBA_CALIB_MAX_ITERATIONS 1
#define LVBA_CALIB_TOO_FEW_RECORDS 2
#define LVBA_CALIB_DEGENERATE 3
typedef struct lvba_calib_opts {
    int32_t max_iterations;  /* 20 */
    int32_t loss_kind;       /* LVBA_LOSS_HUBER */
    int64_t min_records;     /* 100 */
    double loss_scale_px;    /* 2.0 */
    double max_error_px;     /* 0 = no gate */
    double min_eig_ratio;    /* 1e-6 */
    double eps_rot;          /* 1e-10 rad */
    double eps_trans;        /* 1e-10 m */
    int64_t reserved;        /* 0 */
} lvba_calib_opts;           /* 64 bytes */
void    lvba_calib_default_opts(lvba_calib_opts *o);
int32_t lvba_calib_extrinsic(int32_t device, int32_t n_images, const double *body_poses, const double *intr, int32_t n_pairs,
                             const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair, const float *uv_a,
                             const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const lvba_calib_opts *o,
                             double *Rci_out, double *tci_out, int32_t *status, int32_t *iterations, int64_t *n_used, double *rmse_px,
                             double *cost, int32_t *n_held, double *eigenvalues, double *eigenvectors, double *information);
int32_t lvba_calib_linearize(int32_t device, int32_t n_images, const double *body_poses, const double *intr, int32_t n_pairs,
                             const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair, const float *uv_a,
                             const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const lvba_calib_opts *o, double *H,
                             double *g, double *cost, int64_t *n_used, double *sum_sq);

/* ---- the camera-LiDAR time offset as a seventh parameter of the extrinsic refinement (opt-in; DESIGN.md §10o "time offset")
 *   The rule above with one more unknown, td (seconds): the image stamped t was taken at t + td.  Everything not named here is
 *   the 6-parameter rule's, unchanged; restated in numpy in tests/calib_td_oracle.py.  fp64, no contraction; outside the loss only
 *   +, -, *, / and sqrt: a record's terms are the same bits under g++, numpy and gfx950.
 *   New input.  body_twists [n_images][6], a row (om, v) per image: om the body-frame angular velocity (rad/s), v the world-frame
 *     linear velocity (m/s), each taken as constant around its image.
 *   Body pose of image j at td.  th = td om, s = 1 + ((th0^2 + th1^2) + th2^2) / 4, C = I + ([th]x + [th]x^2 / 2) / s (the Cayley
 *     map: an exact rotation about om by 2 atan(td |om| / 2), no sin or cos, whose bits differ between libms); R_j(td) = R_j C,
 *     P_j(td) = P_j + td v_j.
 *   Pair table, per job and per iteration, 21 doubles per (job, pair): A(td) = (R_ab | p_ab) of the two poses at td (12);
 *     om'_a and om'_b with om' = om / (1 + td^2 |om|^2 / 4), the exact rate of the Cayley rotation (dC/dtd = C [om']x); dv =
 *     R_a(td)^T (v_b - v_a).
 *   Record.  r, the first six entries of both Jacobian rows and the loss are the 6-parameter rule's at A(td); counting, gate and
 *     loss are unchanged.  With its q = R^T (Xb - t), w = R_ab q + p_ab and a_k = R^T g_k (g_k the gradient of r_k by Xc):
 *       dw = (R_ab (om'_b x q) - om'_a x w) + dv,   J_k[6] = (a_k0 dw0 + a_k1 dw1) + a_k2 dw2.
 *   Sums.  LVBA_CALIB_TD_SUMS = 39: H upper triangle by row (28), g (7), cost, the count, sum |r|^2, sum rho'.
 *   Step.  The 6-parameter step at n = 7, order (om, up, td): eigenvalues ascending, direction k HELD where not lambda_k >
 *     min_eig_ratio lambda_max, the step in the free span summed in ascending k, the same retraction and td <- td + d[6].
 *     CONVERGED also needs |d[6]| <= eps_td_s (default 1e-10 s, on eps_rot's reasoning).  The DEGENERATE floor is unchanged.
 *     LVBA_CALIB_TD_OUT_OF_RANGE: a step would leave |td| > max_abs_td_s (default 0.2 s: beyond it a constant twist is no
 *     description of the motion; not tuned on data).  That step is not applied and the job returns its start values (Rci, tci,
 *     td0) bit for bit; n_used, rmse_px, cost, the eigen-decomposition and information are of the linearisation the step came from.
 *     Twists that are all zero leave J[6] exactly 0: the job returns the 6-parameter call's extrinsic, status and iterations, td0
 *     unchanged, and one more held direction.  A body whose twist is the same in its own frame at every image (poses exp(k dt xi))
 *     has an A(td) that does not depend on td: the td axis is held beside the screw's two.
 *   Jobs.  Each job has its own (Rci, tci, td0); lock-step over the same records; a job's bytes depend neither on the batch nor
 *     on its place in it.
 *   lvba_calib_extrinsic_td: lvba_calib_extrinsic's arguments plus body_twists and td0 [n_jobs]; its outputs plus td_out
 *     [n_jobs], with eigenvalues [7], eigenvectors [49] (order (om, up, td)) and information [49] per job.
 *   lvba_calib_linearize_td: H [n_jobs][49], g [7], cost, n_used, sum_sq at (Rci, tci, td0), no step.
 *   LVBA_ERR_ARG (nothing written): everything lvba_calib_extrinsic refuses; null or non-finite twists; a null, non-finite or
 *   out-of-range td0 (|td0| > max_abs_td_s); eps_td_s negative or NaN; max_abs_td_s not > 0.  lvba_version() is unchanged; a client
 *   detects these calls by looking lvba_calib_extrinsic_td up. */
#define LVBA_CALIB_TD_OUT_OF_RANGE 4
#define LVBA_CALIB_TD_SUMS 39
typedef struct lvba_calib_td_opts {
    lvba_calib_opts calib;   /* lvba_calib_default_opts */
    double eps_td_s;         /* 1e-10 s */
    double max_abs_td_s;     /* 0.2 s */
    int64_t reserved;        /* 0 */
} lvba_calib_td_opts;        /* 88 bytes */
void    lvba_calib_td_default_opts(lvba_calib_td_opts *o);
int32_t lvba_calib_extrinsic_td(int32_t device, int32_t n_images, const double *body_poses, const double *body_twists, const double *intr,
                                int32_t n_pairs, const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair,
                                const float *uv_a, const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const double *td0,
                                const lvba_calib_td_opts *o, double *Rci_out, double *tci_out, double *td_out, int32_t *status,
                                int32_t *iterations, int64_t *n_used, double *rmse_px, double *cost, int32_t *n_held, double *eigenvalues,
                                double *eigenvectors, double *information);
int32_t lvba_calib_linearize_td(int32_t device, int32_t n_images, const double *body_poses, const double *body_twists, const double *intr,
                                int32_t n_pairs, const int32_t *img_a, const int32_t *img_b, int64_t n_records, const int32_t *pair,
                                const float *uv_a, const double *Xb, int32_t n_jobs, const double *Rci, const double *tci, const double *td0,
                                const lvba_calib_td_opts *o, double *H, double *g, double *cost, int64_t *n_used, double *sum_sq);

/* ---- multi-view colour fusion and photometric consistency of the map (opt-in)
 *   Every map point is projected into every image that sees it, with the occlusion test of the co-visibility stage; the colour is
 *   sampled there; the mean over the views is the fused colour and the spread is the photometric consistency: a number without
 *   ground truth that drops when cameras, extrinsic and trajectory agree with the images -- to the cameras what the mean map
 *   entropy is to the LiDAR poses.  The rule below is this project's own definition, restated in numpy in tests/photo_oracle.py;
 *   it is NOT pinned against anything.
 *   Inputs.  n world points xyz [n][3] (float, host memory; the coloured map's own points are the intended input), n_images images
 *     of width x height, ONE camera model intr = (fx, fy, cx, cy, k1, k2, p1, p2), and optionally a depth set with the same image
 *     count and size on the same device, which the caller keeps alive for as long as the handle.  Images arrive in any number of
 *     lvba_photo_add_images calls: call (first, n) brings images first .. first + n - 1 with Rcw [n][9], tcw [n][3] (T_cam<-world)
 *     and bgr [n][height][width][3] bytes; an image index may be added at most once per handle.
 *   Sample of point X = (double) of the floats in image j (a point with a non-finite coordinate is never sampled).
 *     fate = covis_fate of csrc/covis_device.h, unchanged, with occlusion = a depth set was given, occlusion_rel, occlusion_abs.
 *     Sampled iff fate is SEEN, or SEEN_HOLE (no depth return at the pixel) and holes != 0; and, where max_depth > 0, also
 *     Z <= max_depth, Z = ((R6 X0 + R7 X1) + R8 X2) + t2, the expression the projection evaluates.
 *     (u, v) = the projection's doubles, in [0, width - 1) x [0, height - 1).  x = floor(u), y = floor(v),
 *     a = (int)floor((u - x) 256.0), b likewise from v: exact in fp64.  Texel weights (256 - a)(256 - b), a (256 - b), (256 - a) b,
 *     a b of the texels (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1); they sum to 65 536.  Per channel c = sum weight byte
 *     (int32, at most 255 65 536) and c16 = (c + 128) >> 8, in units of 1/256 grey level, at most 65 280.  Everything after the
 *     projection is integer arithmetic.
 *   Per point, over all images added so far: n_views (int32), S1 [3] = sum c16 (uint32), S2 [3] = sum c16^2 (int64), channels in
 *     the image's order b, g, r.  With n_images <= 32 768: S1 <= 32 768 65 280 < 2^31 and n S2 - S1^2 <= 4.6e18 < 2^63.  The sums
 *     are integers: they do not depend on how the images are split over calls, on the order of the calls, or on the batching.
 *   Finish, per point with n = n_views.  rgb: per channel (2 S1 + 256 n) / (512 n) in integer division (the round-half-up mean),
 *     written r g b as lvba_colorize_download writes; 0 0 0 at n = 0.  sigma (double): with N_c = n S2_c - S1_c^2, an exact
 *     non-negative integer,  sigma = sqrt((((double)N_b + (double)N_g) + (double)N_r) / (3.0 * 65536.0 * (double)(n n)))
 *     evaluated as written, no contraction: the RMS over the channels of the per-channel standard deviation across the views, in
 *     grey levels.  NaN where n_views < min_views.
 *   Summary.  n_points; n_seen: points with n_views >= 1; n_valid: points with n_views >= min_views; n_samples = sum n_views;
 *     mean_sigma over the valid points, an fp64 sum in a fixed order of the library's own (a tree per workgroup of 256 points,
 *     the workgroups' shares added in index order on the host), so two calls give the same bytes, NaN without a valid point;
 *     mean_views = n_samples / n_seen (NaN at n_seen = 0); ms [4]: device time of the upload, the sample pass, the finish (all
 *     three accumulated over the calls so far) and the time of this call's download.
 *   lvba_photo_finish: each of n_views [n], rgb [n][3], sigma [n] may be NULL; it may be called more than once, and more images
 *     may follow.  lvba_photo_sums: the raw sums n_views [n], s1 [n][3] (uint32), s2 [n][3] (int64), each may be NULL.
 *   Options (NULL: the defaults; none of them is tuned on recorded data): occlusion_rel 0.05 and occlusion_abs 0.1 (the
 *     co-visibility stage's), max_depth 0 (none), holes 0 (a sample needs a depth return), min_views 2, max_batch_images 0 (the
 *     images resident at a time: by the free device memory, as the coloriser does).
 *   LVBA_ERR_ARG, before any device work, outputs untouched and the handle still valid: a null pointer; n < 0 or n >= 2^32; width
 *   or height < 2; n_images < 1 or > 32 768; a depth set of another image count, size or device; non-finite intrinsics or focal
 *   lengths <= 0; non-finite cameras; occlusion_rel, occlusion_abs or max_depth negative or non-finite; min_views < 2;
 *   max_batch_images < 0; (first, n) outside [0, n_images); an image index added twice.
 *   lvba_photo_free destroys the handle (it carries that name because the Python binding's test of handle owners lists the
 *   _destroy symbols one by one).  lvba_version() is unchanged; a client detects these calls by looking lvba_photo_create up. */
typedef struct lvba_photo_s *lvba_photo_t;
typedef struct lvba_photo_opts {
    double occlusion_rel;     /* 0.05 */
    double occlusion_abs;     /* 0.1 m */
    double max_depth;         /* 0 = none */
    int32_t holes;            /* 0 */
    int32_t min_views;        /* 2; >= 2 */
    int32_t max_batch_images; /* 0 = by free memory */
    int32_t reserved;         /* 0 */
} lvba_photo_opts;            /* 40 bytes */
typedef struct lvba_photo_summary {
    int64_t n_points, n_seen, n_valid, n_samples;
    double mean_sigma, mean_views;
    double ms[4];
} lvba_photo_summary;         /* 80 bytes */
void    lvba_photo_default_opts(lvba_photo_opts *o);
int32_t lvba_photo_create(int32_t device, int64_t n, const float *xyz, int32_t n_images, int32_t width, int32_t height,
                          const double *intr, lvba_depth_t depth, const lvba_photo_opts *o, lvba_photo_t *out);
int32_t lvba_photo_add_images(lvba_photo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr);
int32_t lvba_photo_finish(lvba_photo_t h, lvba_photo_summary *summary, int32_t *n_views, uint8_t *rgb, double *sigma);
int32_t lvba_photo_sums(lvba_photo_t h, int32_t *n_views, uint32_t *s1, int64_t *s2);
void    lvba_photo_free(lvba_photo_t h);

/* ---- photometric camera alignment against the coloured map (opt-in)
 *   The direct method: the map's colours are held fixed and each camera is moved until its image agrees with them.  Alternated
 *   with the colour fusion above it is the colour-map optimisation of Zhou & Koltun (SIGGRAPH 2014); one image against a reference
 *   it was not fused from is feature-free localisation against the coloured map.  The rule below is this project's own
 *   definition, restated in numpy in tests/palign_oracle.py; it is NOT pinned against anything.  csrc/palign_device.h writes every
 *   scalar expression once, in a fixed order and without contraction: a sample's residuals, rows and weights are the same bits
 *   under g++, numpy and gfx950; the sums over the samples are a tree on the device and are held to the summation bound.
 *   Inputs.  n world points xyz [n][3] (float), per point a reference colour ref16 [n][3] (uint16; channels b, g, r in 1/256 grey
 *     level, the fusion's unit: from its sums (2 S1 + n_views) / (2 n_views) in integers) and a validity byte valid [n] (0: the
 *     point is never sampled); n_images images of width x height as uploaded (bgr, 3 bytes a texel), ONE camera model intr = (fx,
 *     fy, cx, cy, k1, k2, p1, p2), initial Rcw [9], tcw [3] (T_cam<-world) per image, and optionally a depth set with the same
 *     image count and size on the same device, kept alive by the caller: the occlusion test.  The depth images are those of the
 *     INITIAL poses; they are not rendered again inside the iteration.
 *   Sample of point X in image j at pose (R, t).  Exactly the colour fusion's: the same fate, max_depth and holes, the same (u, v),
 *     x, y, a, b and c16 [3].  In addition the bilinear gradient from the same four texels t00 = (y, x), t10 = (y, x + 1), t01 =
 *     (y + 1, x), t11 = (y + 1, x + 1), per channel, in grey levels per pixel:
 *       gu = ((256 - b)(t10 - t00) + b (t11 - t01)) / 256,  gv = ((256 - a)(t01 - t00) + a (t11 - t10)) / 256
 *     with integer numerators and one division.
 *   Residual per channel.  r = (c16 - ref16) / 256, in grey levels.
 *   Jacobian under the resection's left perturbation (R <- (I + [om]x) R re-orthonormalised through a unit quaternion, t <- t +
 *     om x t + up, order (om, up)): Xc = R X + t moves by om x Xc + up.  With Jpi the 2 x 3 Jacobian of the projection at Xc, the
 *     distortion included, and q = gu Jpi[0] + gv Jpi[1], the channel's row is (Xc x q, q).
 *   Loss.  loss_eval of csrc/visual_loss.h on s = r^2, per channel, at loss_scale grey levels, kinds LVBA_LOSS_*: weight rho', cost
 *     rho / 2.  Default Huber at 10 grey levels: the value of the numpy prototype this stage started from, not tuned on data.
 *   Sums per image (LVBA_PALIGN_SUMS = 31 doubles): H = sum rho' J^T J, upper triangle by row (21); g = sum rho' J^T r (6); cost =
 *     sum rho / 2; n_samples (a sample counts once, its three channels are three terms of the other sums); sum r^2; sum rho'.
 *   Step: Levenberg-Marquardt per image, all images of a call in lock-step.  (H + lambda diag(max(H_aa, 1e-12))) d = -g by a 6 x 6
 *     LDL^T; the trial pose is the perturbation d applied to the current pose.  One linearisation at the trial pose gives its mean
 *     cost m = cost / n_samples; the trial is accepted iff n_samples >= min_samples and m_trial < m_current.  Accepted: the trial
 *     and its H, g become current and lambda <- max(lambda / 3, 1e-9).  Rejected: lambda <- 4 lambda.  lambda starts at 1e-3.  A
 *     pass is one linearisation, whatever its outcome: the first is at the initial pose, and an image takes at most
 *     max_iterations passes (default 15).
 *   Status per image.  LVBA_PALIGN_CONVERGED: an accepted step with |om| <= eps_rot (1e-7) and |up| <= eps_trans (1e-6 m).
 *     LVBA_PALIGN_MAX_ITERATIONS: max_iterations passes without converging; the current pose is returned.
 *     LVBA_PALIGN_TOO_FEW_SAMPLES: fewer than min_samples (default 200) samples at the initial pose.  LVBA_PALIGN_DEGENERATE: a
 *     diagonal entry of H is not > 0, a pivot of the damped system is not > 0, or the step is not finite.
 *     LVBA_PALIGN_OUT_OF_BOUNDS: an accepted pose is more than max_rotation_deg (default 5 degrees) or max_translation (default
 *     0.5 m, of the camera centre) from the initial one.  With the last three the initial pose is returned bit for bit, and rmse,
 *     cost, n_samples and information are those of the initial pose.  A finished image is skipped by the later passes.  What an
 *     image returns depends neither on the other images of the call, nor on its place among them, nor on the batching.
 *   lvba_palign_align, images first .. first + n - 1 (first only selects the depth images): per image Rcw_out [9], tcw_out [3],
 *     status, iterations (passes), accepted (steps), n_samples, rmse = sqrt(sum r^2 / (3 n_samples)) in grey levels at the initial
 *     (rmse_initial) and at the returned pose (0 without a sample), cost, information [36] = H at the returned pose.
 *   lvba_palign_linearize: the diagnostic call, one evaluation per image at the given poses and no step: sums [n][31], the
 *     per-image photometric residual.  lvba_palign_profile: ms [3], the device time of the uploads, the linearisation passes and
 *     the steps, accumulated over the handle's calls.
 *   Options (NULL: the defaults; none is tuned on recorded data): occlusion_rel, occlusion_abs, max_depth, holes and
 *     max_batch_images as in lvba_photo_opts.
 *   LVBA_ERR_ARG, before any device work, outputs untouched and the handle still valid: a null pointer; n < 0 or n >= 2^32; width
 *   or height < 2; n_images < 1 or > 32 768; a depth set of another image count, size or device; non-finite intrinsics or focal
 *   lengths <= 0; non-finite cameras; (first, n) outside [0, n_images); max_iterations outside 1 .. 1000; a negative or non-finite
 *   threshold (occlusion_rel, occlusion_abs, max_depth, eps_rot, eps_trans, max_rotation_deg -- also above 180 --,
 *   max_translation); an unknown loss; a loss scale that is not > 0; min_samples < 6; max_batch_images < 0.
 *   lvba_palign_free destroys the handle.  lvba_version() is unchanged; a client detects these calls by looking lvba_palign_create
 *   up. */
#define LVBA_PALIGN_CONVERGED 0
#define LVBA_PALIGN_MAX_ITERATIONS 1
#define LVBA_PALIGN_TOO_FEW_SAMPLES 2
#define LVBA_PALIGN_DEGENERATE 3
#define LVBA_PALIGN_OUT_OF_BOUNDS 4
#define LVBA_PALIGN_SUMS 31
typedef struct lvba_palign_s *lvba_palign_t;
typedef struct lvba_palign_opts {
    double occlusion_rel;     /* 0.05 */
    double occlusion_abs;     /* 0.1 m */
    double max_depth;         /* 0 = none */
    double loss_scale;        /* 10 grey levels */
    double eps_rot;           /* 1e-7 rad */
    double eps_trans;         /* 1e-6 m */
    double max_rotation_deg;  /* 5 */
    double max_translation;   /* 0.5 m */
    int32_t holes;            /* 0 */
    int32_t loss_kind;        /* LVBA_LOSS_HUBER */
    int32_t min_samples;      /* 200; >= 6 */
    int32_t max_iterations;   /* 15 */
    int32_t max_batch_images; /* 0 = by free memory */
    int32_t reserved;         /* 0 */
} lvba_palign_opts;           /* 88 bytes */
void    lvba_palign_default_opts(lvba_palign_opts *o);
int32_t lvba_palign_create(int32_t device, int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int32_t n_images,
                           int32_t width, int32_t height, const double *intr, lvba_depth_t depth, const lvba_palign_opts *o,
                           lvba_palign_t *out);
int32_t lvba_palign_linearize(lvba_palign_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                              double *sums);
int32_t lvba_palign_align(lvba_palign_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                          double *Rcw_out, double *tcw_out, int32_t *status, int32_t *iterations, int32_t *accepted, int64_t *n_samples,
                          double *rmse_initial, double *rmse, double *cost, double *information);
int32_t lvba_palign_profile(lvba_palign_t h, double *ms);
void    lvba_palign_free(lvba_palign_t h);

/* ---- per-image exposure compensation of the colour fusion (opt-in)
 *   The fusion above assumes that a surface has the same grey level in every image.  A camera with auto-exposure and auto white
 *   balance breaks that: the spread then measures exposure differences, which no pose change removes, and the fused colour shows
 *   seams where the set of images that see a point changes.  This stage estimates a gain and an offset per image and channel
 *   against the fused colours, and the fusion applies them.  The rule below is this project's own definition (the reference takes
 *   one pixel of one image and has nothing of the kind), restated with Python integers in tests/expo_oracle.py; it is NOT pinned
 *   against anything.  csrc/expo_device.h writes every scalar piece once.  Everything after the projection is integer arithmetic.
 *   Gains.  int64_t gains [n_images][3][2] = (A, B) per image and channel, in the image's order b, g, r.  A in units of 2^-16, B
 *     in units of 2^-16 of 1/256 grey level; the identity is (65536, 0).  The compensated sample of c16 is
 *       c' = clamp(floor((A c16 + B + 32768) / 65536), 0, 65280)     in int64, floor towards minus infinity.
 *     The clamp keeps the fusion's bounds on S1, S2 and n S2 - S1^2 as they are.
 *   Fusion with gains, lvba_photo_add_images_gains: gains [n][3][2] are those of the images of this call; the sample is the
 *     fusion's, except that c' takes the place of c16 in the sums.  gains == NULL or all identity gives the bytes of
 *     lvba_photo_add_images.  lvba_photo_add_images, lvba_photo_opts and lvba_photo_summary are unchanged.
 *   Estimation sums, lvba_expo_sums, per image against a reference ref16 [n][3] / valid [n] -- what lvba_palign_create takes, every
 *     ref16 at most 65 280 -- under the gains gains_in [n][3][2] (NULL: identity).  A point with valid = 0 is skipped.  A valid point
 *     is located in image j exactly as the fusion locates it (the same fate, max_depth and holes, the same (u, v), a, b and
 *     texels).  Channel k of a located sample is USED iff (1) each of the four texel bytes of channel k lies in [sat_lo, sat_hi]
 *     -- a clipped texel breaks the affine model -- and (2) where gate > 0, |c' - ref| <= gate 256 with c' under gains_in -- a
 *     point coloured through a wrong occlusion decision or a specular highlight stays out.  Both are integer comparisons.
 *     LVBA_EXPO_SUMS = 20 values of uint64 per image: per channel k at [6 k]: n, sum c, sum ref, sum c^2, sum c ref,
 *     sum (c' - ref)^2 over the used terms, c = c16 raw; then [18] n_located, the located samples, and [19] the channel terms
 *     that passed (1) and that the gate refused.  With fewer than 2^32 points every sum stays below 2^32 65280^2 < 2^64, because
 *     65280^2 < 2^32.  The sums are integers: nothing depends on the batching or on how the images are split over calls.
 *   Solve, lvba_expo_solve: host arithmetic only, pure integer arithmetic, in 128 bits where products need it: C++, Python
 *     integers and any caller give the same bytes.  Per image and channel  D = n sum c^2 - (sum c)^2,  N = n sum c ref - sum c sum ref.
 *       LVBA_EXPO_AFFINE (default):  A = floor((N 2^16 + D / 2) / D),  B = floor(((sum ref 2^16 - A sum c) 2 + n) / (2 n))
 *       LVBA_EXPO_GAIN:              A = floor((sum c ref 2^16 + sum c^2 / 2) / sum c^2),  B = 0
 *     (D / 2 and sum c^2 / 2 in integer division of non-negative numbers).  Per channel, in this order:
 *       n < min_samples                                              -> LVBA_EXPO_TOO_FEW_SAMPLES
 *       affine and D <= n^2 (min_spread 256)^2: the view is too flat to tell a gain from an offset
 *                                                                    -> LVBA_EXPO_FALLBACK_GAIN, the channel takes the gain-only form
 *       the gain-only form with sum c^2 = 0; A outside [min_gain, max_gain]; |B| above max_offset
 *                                                                    -> LVBA_EXPO_OUT_OF_BOUNDS
 *       else LVBA_EXPO_OK.  min_gain and max_gain are compared as floor(x 2^16 + 0.5), max_offset as floor(x 2^24 + 0.5).
 *     Status per image: the worst of its three channels (the largest value).  With TOO_FEW_SAMPLES or OUT_OF_BOUNDS all three
 *     channels of the image are the identity.
 *   Gauge.  Alternating the fusion and the solve fixes the gains only up to one global affine map per channel; it is set so that
 *     the mean gain is 1 and the mean offset 0, per channel over the n_ok images that are OK or FALLBACK_GAIN:
 *       S = floor((n_ok 2^32 + sum A / 2) / sum A);  A <- floor((A S + 2^15) / 2^16);  B <- floor((B S + 2^15) / 2^16) - T
 *     with T = floor((2 sum B + n_ok) / (2 n_ok)) of the scaled B, the round-half-up mean.  The spread then stays in the grey levels
 *     of the average image and remains comparable with the uncompensated number.  An image whose gauged A is outside
 *     [2^14, 2^18] or whose |B| is above 2^16 65280 -- gains the fusion would refuse -- becomes OUT_OF_BOUNDS with the identity.
 *   lvba_expo_profile: ms [2], the device time of the uploads and of the sums passes, accumulated over the handle's calls.
 *   Options (NULL: the defaults; all of them are this library's choice and none is tuned on recorded data): occlusion_rel,
 *     occlusion_abs, max_depth, holes and max_batch_images as in lvba_photo_opts; model LVBA_EXPO_AFFINE; sat_lo 4, sat_hi 251;
 *     gate 30 grey levels (0: off); min_samples 200; min_spread 2 grey levels; min_gain 0.25, max_gain 4, max_offset 64 grey levels.
 *   LVBA_ERR_ARG, before any device work, outputs untouched and the handle still valid: a null pointer (gains and gains_in may
 *   be NULL); n < 0 or n >= 2^32; width or height < 2; n_images < 1 or > 32 768 (the solve: < 0); a depth set of another image
 *   count, size or device; non-finite intrinsics or focal lengths <= 0; non-finite cameras; (first, n) outside [0, n_images); an
 *   image index added twice (the fusion); occlusion_rel, occlusion_abs or max_depth negative or non-finite; max_batch_images < 0;
 *   an unknown model; sat_lo < 0, sat_hi > 255 or sat_lo > sat_hi; gate or min_spread outside 0 .. 255; min_samples < 2;
 *   min_gain outside [0.25, 1]; max_gain outside [1, 4]; max_offset outside [0, 255]; a ref16 above 65 280; an A outside
 *   [2^14, 2^18] or a |B| above 2^16 65280 in gains or gains_in; sums given to the solve that fewer than 2^32 samples of at most
 *   65 280 cannot have.
 *   lvba_expo_free destroys the handle.  lvba_version() is unchanged; a client detects the stage by looking lvba_expo_create up. */
#define LVBA_EXPO_OK 0
#define LVBA_EXPO_FALLBACK_GAIN 1
#define LVBA_EXPO_TOO_FEW_SAMPLES 2
#define LVBA_EXPO_OUT_OF_BOUNDS 3
#define LVBA_EXPO_AFFINE 0
#define LVBA_EXPO_GAIN 1
#define LVBA_EXPO_SUMS 20
typedef struct lvba_expo_s *lvba_expo_t;
typedef struct lvba_expo_opts {
    double occlusion_rel;     /* 0.05 */
    double occlusion_abs;     /* 0.1 m */
    double max_depth;         /* 0 = none */
    double min_gain;          /* 0.25 */
    double max_gain;          /* 4 */
    double max_offset;        /* 64 grey levels */
    int32_t holes;            /* 0 */
    int32_t model;            /* LVBA_EXPO_AFFINE */
    int32_t sat_lo;           /* 4 */
    int32_t sat_hi;           /* 251 */
    int32_t gate;             /* 30 grey levels; 0 = off */
    int32_t min_samples;      /* 200; >= 2 */
    int32_t min_spread;       /* 2 grey levels */
    int32_t max_batch_images; /* 0 = by free memory */
} lvba_expo_opts;             /* 80 bytes */
void    lvba_expo_default_opts(lvba_expo_opts *o);
int32_t lvba_expo_create(int32_t device, int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int32_t n_images,
                         int32_t width, int32_t height, const double *intr, lvba_depth_t depth, const lvba_expo_opts *o, lvba_expo_t *out);
int32_t lvba_expo_sums(lvba_expo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                       const int64_t *gains_in, uint64_t *sums);
int32_t lvba_expo_solve(int32_t n_images, const uint64_t *sums, const lvba_expo_opts *o, int64_t *gains, int32_t *status);
int32_t lvba_expo_profile(lvba_expo_t h, double *ms);
void    lvba_expo_free(lvba_expo_t h);
int32_t lvba_photo_add_images_gains(lvba_photo_t h, int32_t first, int32_t n, const double *Rcw, const double *tcw, const uint8_t *bgr,
                                    const int64_t *gains);

/* ---- the undistorted images of the COLMAP export (opt-in)
 *   The reference's end product names an image k.jpg per row of images.txt and writes it undistorted (DatasetIO::undistortImage,
 *   src/dataset_io.cpp:15-26: initUndistortRectifyMap with newK = K, then remap(INTER_LINEAR)); the poses of images.txt belong to
 *   that pinhole image, not to the raw Brown-Conrady one.  This stage writes those pixels.  The rule below is this project's own
 *   definition, restated in numpy in tests/undistort_oracle.py; it is NOT pinned against OpenCV, whose fixed-point map and weight
 *   table are not restated.  csrc/undistort_device.h writes every scalar piece once.
 *   Inputs: the source camera intr [8] = fx fy cx cy k1 k2 p1 p2 and size w x h, images BGR uint8 [n][h][w][3]; the target
 *     pinhole fx' fy' cx' cy' (fx' = 0: all four from the source, the reference's newK = K) and size w' x h' (0: the source's).
 *   Position.  For target pixel column i, row j:  x = (i - cx') / fx',  y = (j - cy') / fy',  (u, v) = the projection of the
 *     camera-frame point (x, y, 1) through the source camera -- the fusion's own projection, the same doubles: + - * / in fp64 in
 *     a file built without contraction.  The pixel is VALID iff the projection succeeds and 0 <= u < w - 1, 0 <= v < h - 1, the
 *     range the colour fusion samples in.
 *   Colour.  An invalid pixel is `border` in its three bytes and its mask byte is 0 (a valid one's is 255).  Channel k of a valid
 *     pixel: c16 = the fusion's sample at (u, v), 1/256-pixel fractions and integer weights, in 1/256 grey level; with gains,
 *     c16 <- the compensated sample under the image's (A, B) of channel k (§10r above); the byte is (c16 + 128) >> 8, at most 255.
 *     What a pinhole projection reads from the exported image is therefore byte for byte what the fusion read from the raw one.
 *   Two differences from OpenCV's remap: no partial blend with the border in the source's last row and column (such a pixel is
 *     invalid), and fractions of 1/256 pixel, not 1/32.  The polynomial model can fold far outside the image: a target field of
 *     view much wider than the source's shows mirrored content there, as it does under OpenCV; this is left alone.
 *   gains: NULL, or int64 [n][3][2] of the images of the call, as lvba_photo_add_images_gains takes them.  The bytes do not depend
 *     on max_batch_images (default 64, which keeps the stage's device memory small; 0: batches by the free memory, as the
 *     fusion's) or on how the images are split over calls.
 *   lvba_undistort_tile: host only; the kernel's pixels per lane and its tile of the target, the sizes a test puts its cases at.
 *   lvba_undistort_info: each output may be NULL; pinhole [4] = fx' fy' cx' cy' as resolved; n_valid the valid target pixels.
 *   lvba_undistort_map: uv [h'][w'][2] (NaN where invalid) and mask [h'][w'], either may be NULL; a small kernel of its own over
 *     the same position function.  lvba_undistort_profile: ms [3], the device time of the uploads, the kernel and the downloads,
 *     accumulated over the handle's calls.
 *   LVBA_ERR_ARG, before any device work, outputs untouched and the handle still valid: a null pointer (opts, gains and the
 *   outputs named above may be NULL); n < 0; a source or target width or height below 2; non-finite intrinsics or source focal
 *   lengths <= 0; a non-finite target pinhole or a target focal length <= 0 (fx' = 0 alone means the source's); border outside
 *   0 .. 255; max_batch_images < 0; an A outside [2^14, 2^18] or a |B| above 2^16 65280 in gains.
 *   lvba_undistort_free destroys the handle.  lvba_version() is unchanged; a client detects the stage by looking
 *   lvba_undistort_create up. */
typedef struct lvba_undistort_s *lvba_undistort_t;
typedef struct lvba_undistort_opts {
    double fx, fy, cx, cy;    /* the target pinhole; fx = 0: the source's four */
    int32_t out_width;        /* 0 = the source's */
    int32_t out_height;       /* 0 = the source's */
    int32_t border;           /* 0; the grey level of an invalid pixel, 0 .. 255 */
    int32_t max_batch_images; /* 64; 0 = by free memory */
} lvba_undistort_opts;        /* 48 bytes */
void    lvba_undistort_default_opts(lvba_undistort_opts *o);
int32_t lvba_undistort_tile(int32_t *pixels_per_lane, int32_t *tile_width, int32_t *tile_height);
int32_t lvba_undistort_create(int32_t device, int32_t width, int32_t height, const double intr[8], const lvba_undistort_opts *o,
                              lvba_undistort_t *out);
int32_t lvba_undistort_info(lvba_undistort_t h, int32_t *out_width, int32_t *out_height, double pinhole[4], int64_t *n_valid);
int32_t lvba_undistort_images(lvba_undistort_t h, int32_t n, const uint8_t *bgr, const int64_t *gains, uint8_t *bgr_out);
int32_t lvba_undistort_map(lvba_undistort_t h, double *uv, uint8_t *mask);
int32_t lvba_undistort_profile(lvba_undistort_t h, double ms[3]);
void    lvba_undistort_free(lvba_undistort_t h);

#ifdef __cplusplus
}
#endif
#endif /* LVBA_HIP_H */
