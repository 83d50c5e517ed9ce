// calib_td_check.cpp -- csrc/calib_td_device.h compiled for the host (tests/test_calib_td_host.py loads it through ctypes; built by
// tests/host_build.py without contraction): the shifted pose, the pair table's row, the per-record rule with its seventh column,
// the sums in index order and in reversed order, the step, and the whole iteration of one job.
#include <stdint.h>
#include <vector>
#include "../global-lvba_amd/csrc/calib_td_device.h"

using namespace lvba;

static CalTdParams params(const double *p)
{
    // p: fx, fy, max_error_px, loss_scale, min_eig_ratio, eps_rot, eps_trans, min_records, loss_kind, eps_td, max_abs_td
    CalTdParams o{};
    o.cal.fx = p[0]; o.cal.fy = p[1]; o.cal.max_error_px = p[2]; o.cal.loss_scale = p[3]; o.cal.min_eig_ratio = p[4]; o.cal.eps_rot = p[5];
    o.cal.eps_trans = p[6]; o.cal.min_records = (int64_t)p[7]; o.cal.loss_kind = (int32_t)p[8];
    o.eps_td = p[9]; o.max_abs_td = p[10];
    return o;
}

static void sums_of(int64_t n, const double *x, const double *E, const int32_t *pair, const double *xy, const double *Xb, const CalParams &o,
                    int reverse, double *s)
{
    for (int q = 0; q < CAL_TD_NS; ++q) s[q] = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = reverse ? n - 1 - k : k;
        cal_td_record(x, x + 9, E + CAL_TD_ROW * (int64_t)pair[i], xy[2 * i], xy[2 * i + 1], Xb + 3 * i, o, s);
    }
}

static void table_of(int32_t n_pairs, const double *poses, const double *twists, const int32_t *img_a, const int32_t *img_b, double td,
                     double *E)
{
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t a = img_a[p], b = img_b[p];
        cal_td_pair(poses + 12 * a, poses + 12 * b, twists + 6 * a, twists + 6 * b, td, E + CAL_TD_ROW * (int64_t)p);
    }
}

extern "C" {

// out [8]: CAL_TD_N, CAL_TD_NS, CAL_TD_ROW, CAL_TD_WS, CAL_TD_EXT, sizeof(CalTdResult), sizeof(CalTdParams), CAL_TD_OUT_OF_RANGE
void emul_td_constants(int64_t *out)
{
    out[0] = CAL_TD_N; out[1] = CAL_TD_NS; out[2] = CAL_TD_ROW; out[3] = CAL_TD_WS; out[4] = CAL_TD_EXT;
    out[5] = (int64_t)sizeof(CalTdResult); out[6] = (int64_t)sizeof(CalTdParams); out[7] = CAL_TD_OUT_OF_RANGE;
}

void emul_td_shift(int32_t M, const double *poses, const double *twists, double td, double *out)
{
    for (int32_t k = 0; k < M; ++k) cal_td_pose(poses + 12 * (int64_t)k, twists + 6 * (int64_t)k, td, out + 12 * (int64_t)k);
}

void emul_td_pairs(int32_t n_pairs, const double *poses, const double *twists, const int32_t *img_a, const int32_t *img_b, double td, double *E)
{
    table_of(n_pairs, poses, twists, img_a, img_b, td, E);
}

// counted [n], r [n][2], J0, J1 [n][7], rho [n][3]: rows of records that do not count are left as they are
void emul_td_eval(int64_t n, const double *R, const double *t, const double *E, const int32_t *pair, const double *xy, const double *Xb,
                  const double *p, uint8_t *counted, double *r, double *J0, double *J1, double *rho)
{
    const CalTdParams o = params(p);
    for (int64_t i = 0; i < n; ++i)
        counted[i] = cal_td_eval(R, t, E + CAL_TD_ROW * (int64_t)pair[i], xy[2 * i], xy[2 * i + 1], Xb + 3 * i, o.cal, r + 2 * i, J0 + 7 * i,
                                 J1 + 7 * i, rho + 3 * i) ? 1 : 0;
}

// x [13] = (R, t, td); only (R, t) are read: the table E is at the caller's td
void emul_td_sums(int64_t n, const double *x, const double *E, const int32_t *pair, const double *xy, const double *Xb, const double *p,
                  int32_t reverse, double *s)
{
    sums_of(n, x, E, pair, xy, Xb, params(p).cal, reverse, s);
}

// res [3 + 7 + 49]: rmse, cost, n_used, eig, vec; counts [1]: n_held.  x [13] is stepped on RUNNING.
int32_t emul_td_step(const double *s, const double *p, int32_t may_step, double *x, double *res, int32_t *counts)
{
    double ws[CAL_TD_WS];
    CalTdResult out{};
    const int st = cal_td_step(s, params(p), may_step != 0, x, ws, out);
    res[0] = out.rmse; res[1] = out.cost; res[2] = (double)out.n_used;
    for (int k = 0; k < 7; ++k) res[3 + k] = out.eig[k];
    for (int k = 0; k < 49; ++k) res[10 + k] = out.vec[k];
    counts[0] = out.n_held;
    return st;
}

// the whole iteration of one job, every sum in index order (reverse: in reversed order); x [13] in and out (its start values on
// OUT_OF_RANGE, as the library returns them); s [CAL_TD_NS]: the sums of the last linearisation; eigvec [7 + 49] of the last step
int32_t emul_td_solve(int32_t n_pairs, const double *poses, const double *twists, const int32_t *img_a, const int32_t *img_b, int64_t n,
                      const int32_t *pair, const double *xy, const double *Xb, const double *p, int32_t max_it, int32_t reverse, double *x,
                      double *s, int32_t *iterations, int32_t *n_held, double *eigvec)
{
    const CalTdParams o = params(p);
    double ws[CAL_TD_WS], x0[CAL_TD_EXT];
    for (int k = 0; k < CAL_TD_EXT; ++k) x0[k] = x[k];
    std::vector<double> E((size_t)CAL_TD_ROW * (size_t)n_pairs);
    CalTdResult out{};
    int st = CAL_RUNNING, it = 0;
    for (;; ++it) {
        table_of(n_pairs, poses, twists, img_a, img_b, x[12], E.data());
        sums_of(n, x, E.data(), pair, xy, Xb, o.cal, reverse, s);
        st = cal_td_step(s, o, it < max_it, x, ws, out);
        if (st != CAL_RUNNING) break;
    }
    if (st == CAL_TD_OUT_OF_RANGE)
        for (int k = 0; k < CAL_TD_EXT; ++k) x[k] = x0[k];
    *iterations = it;
    *n_held = out.n_held;
    for (int k = 0; k < 7; ++k) eigvec[k] = out.eig[k];
    for (int k = 0; k < 49; ++k) eigvec[7 + k] = out.vec[k];
    return st;
}

} // extern "C"
