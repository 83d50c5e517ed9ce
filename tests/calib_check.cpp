// calib_check.cpp -- csrc/calib_device.h compiled for the host (tests/test_calib_host.py loads it through ctypes; built by
// tests/host_build.py without contraction): the pair transform, the record's target, the per-record rule, the sums in index order
// and in reversed order, the step, and the whole iteration of one job.
#include <stdint.h>
#include <vector>
#include "../global-lvba_amd/csrc/calib_device.h"

using namespace lvba;

static CalParams params(const double *p)
{
    // p: fx, fy, max_error_px, loss_scale, min_eig_ratio, eps_rot, eps_trans, min_records, loss_kind
    CalParams o{};
    o.fx = p[0]; o.fy = p[1]; o.max_error_px = p[2]; o.loss_scale = p[3]; o.min_eig_ratio = p[4]; o.eps_rot = p[5]; o.eps_trans = p[6];
    o.min_records = (int64_t)p[7]; o.loss_kind = (int32_t)p[8];
    return o;
}

static void sums_of(int64_t n, const double *R, const double *t, const double *A, const int32_t *pair, const double *xy, const double *Xb,
                    const CalParams &o, int reverse, double *s)
{
    for (int q = 0; q < CAL_NS; ++q) s[q] = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = reverse ? n - 1 - k : k;
        cal_record(R, t, A + 12 * (int64_t)pair[i], xy[2 * i], xy[2 * i + 1], Xb + 3 * i, o, s);
    }
}

extern "C" {

// out [7]: CAL_NS, CAL_BLOCK, CAL_RUN, CAL_MAX_BLOCKS, CAL_WS, sizeof(CalResult), sizeof(CalParams)
void emul_constants(int64_t *out)
{
    out[0] = CAL_NS; out[1] = CAL_BLOCK; out[2] = CAL_RUN; out[3] = CAL_MAX_BLOCKS; out[4] = CAL_WS; out[5] = (int64_t)sizeof(CalResult);
    out[6] = (int64_t)sizeof(CalParams);
}

int32_t emul_blocks(int64_t n) { return cal_blocks(n); }

void emul_pairs(int32_t n_pairs, const double *poses, const int32_t *img_a, const int32_t *img_b, double *A)
{
    for (int32_t p = 0; p < n_pairs; ++p) cal_pair(poses + 12 * (int64_t)img_a[p], poses + 12 * (int64_t)img_b[p], A + 12 * (int64_t)p);
}

void emul_targets(int64_t n, const double *intr, const float *uv, const double *Xb, double *xy)
{
    const TrkIntr cam = trk_intr_of(intr);
    for (int64_t i = 0; i < n; ++i) cal_target(cam, uv[2 * i], uv[2 * i + 1], Xb + 3 * i, xy[2 * i], xy[2 * i + 1]);
}

// counted [n], r [n][2], J0, J1 [n][6], rho [n][3]: rows of records that do not count are left as they are
void emul_eval(int64_t n, const double *R, const double *t, const double *A, const int32_t *pair, const double *xy, const double *Xb,
               const double *p, uint8_t *counted, double *r, double *J0, double *J1, double *rho)
{
    const CalParams o = params(p);
    for (int64_t i = 0; i < n; ++i)
        counted[i] = cal_eval(R, t, A + 12 * (int64_t)pair[i], xy[2 * i], xy[2 * i + 1], Xb + 3 * i, o, r + 2 * i, J0 + 6 * i, J1 + 6 * i,
                              rho + 3 * i) ? 1 : 0;
}

void emul_sums(int64_t n, const double *R, const double *t, const double *A, const int32_t *pair, const double *xy, const double *Xb,
               const double *p, int32_t reverse, double *s)
{
    sums_of(n, R, t, A, pair, xy, Xb, params(p), reverse, s);
}

// res [3 + 6 + 36]: rmse, cost, n_used, eig, vec; counts [2]: n_held, (unused).  R, t are retracted on RUNNING.
int32_t emul_step(const double *s, const double *p, int32_t may_step, double *R, double *t, double *res, int32_t *counts)
{
    double ws[CAL_WS];
    CalResult out{};
    const int st = cal_step(s, params(p), may_step != 0, R, t, ws, out);
    res[0] = out.rmse; res[1] = out.cost; res[2] = (double)out.n_used;
    for (int k = 0; k < 6; ++k) res[3 + k] = out.eig[k];
    for (int k = 0; k < 36; ++k) res[9 + k] = out.vec[k];
    counts[0] = out.n_held;
    return st;
}

// eigenvalues unsorted in lam [6], V [36] with the vector of lam[k] in column k
void emul_jacobi(const double *H, double *lam, double *V)
{
    double A[36];
    for (int k = 0; k < 36; ++k) A[k] = H[k];
    cal_jacobi(A, V, 6);
    for (int k = 0; k < 6; ++k) lam[k] = A[7 * k];
}

// the whole iteration of one job, every sum in index order (reverse: in reversed order); R, t in and out; s [CAL_NS]: the sums of
// the last linearisation; returns the status, *iterations the steps applied
int32_t emul_solve(int64_t n, const double *A, const int32_t *pair, const double *xy, const double *Xb, const double *p, int32_t max_it,
                   int32_t reverse, double *R, double *t, double *s, int32_t *iterations, int32_t *n_held)
{
    const CalParams o = params(p);
    double ws[CAL_WS];
    CalResult out{};
    int st = CAL_RUNNING, it = 0;
    for (;; ++it) {
        sums_of(n, R, t, A, pair, xy, Xb, o, reverse, s);
        st = cal_step(s, o, it < max_it, R, t, ws, out);
        if (st != CAL_RUNNING) break;
    }
    *iterations = it;
    *n_held = out.n_held;
    return st;
}

} // extern "C"
