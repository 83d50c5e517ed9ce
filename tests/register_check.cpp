// register_check.cpp -- csrc/register_device.h compiled for the host (tests/test_register_host.py): the per-point rule over a
// cloud with given planes, and the per-job step.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include "../global-lvba_amd/csrc/register_device.h"

using namespace lvba;

static RegParams params(double max_distance, int64_t min_inliers, double min_eigenvalue, double tol_rot, double tol_pos, int loss_kind,
                        double loss_scale)
{
    RegParams o;
    o.max_distance = max_distance; o.min_eigenvalue = min_eigenvalue; o.tol_rot = tol_rot; o.tol_pos = tol_pos;
    o.loss_scale = loss_scale; o.min_inliers = min_inliers; o.loss_kind = loss_kind;
    return o;
}

extern "C" {

int emul_sizes(int *ns, int *ws) { *ns = REG_NS; *ws = REG_WS; return 0; }

// sums [REG_NS] of the points in index order; world [m][3], resid [m] (0 where no plane), inlier [m]
void emul_linearize(int64_t m, const float *pts, const double *T, const double *plane, const uint8_t *found, double max_distance,
                    int loss_kind, double loss_scale, double *sums, double *world, double *resid, uint8_t *inlier)
{
    const RegParams o = params(max_distance, 0, 0.0, 0.0, 0.0, loss_kind, loss_scale);
    for (int q = 0; q < REG_NS; ++q) sums[q] = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double w[3];
        reg_world(T, p, w);
        for (int a = 0; a < 3; ++a) world[3 * i + a] = w[a];
        resid[i] = 0.0; inlier[i] = 0;
        if (!found[i]) continue;
        resid[i] = reg_residual(w, plane + 4 * i);
        inlier[i] = reg_point(T, p, w, plane + 4 * i, o, sums) ? 1 : 0;
    }
}

// one step from sums; T [12] in and out; returns the state
int emul_step(const double *sums, double max_distance, int64_t min_inliers, double min_eigenvalue, double tol_rot, double tol_pos, double *T,
              double *min_eig, double *rmse)
{
    const RegParams o = params(max_distance, min_inliers, min_eigenvalue, tol_rot, tol_pos, 0, 0.0);
    double ws[REG_WS];
    return reg_step(sums, o, T, ws, min_eig, rmse);
}

double emul_jacobi_min(double *A, int n) { return reg_jacobi_min(A, n); }
int emul_ldlt_solve(double *A, double *b, int n) { return reg_ldlt_solve(A, b, n) ? 1 : 0; }

} // extern "C"
