// posegraph_check.cpp -- csrc/posegraph_device.h compiled for the host (tests/test_posegraph_host.py loads it with ctypes): the
// odometry record, an edge's weighted lin record and cost, and the retraction, one edge at a time.
#include "../global-lvba_amd/csrc/posegraph_device.h"
#include "../global-lvba_amd/csrc/balm_math.h"

using namespace lvba;

extern "C" {

// rec [72] = meas | oi | oj | L
void pgc_odometry(const double *Xi, const double *Xj, double sigma_rot, double sigma_pos, double *rec)
{
    pg_odometry_record(Xi, Xj, 1.0 / sigma_rot, 1.0 / sigma_pos, rec, rec + 12, rec + 24, rec + 36);
}

// lin [128], out [2] = cost | weight
void pgc_lin(int kind, const double *rec, const double *Ti, const double *Tj, int flip, int loss_kind, double loss_scale, double *lin, double *out)
{
    for (int a = 0; a < PL_LIN; ++a) lin[a] = 0.0;
    if (kind == PRIOR_POSE) out[0] = pg_edge_lin(PRIOR_POSE, rec, rec + 12, rec + 24, rec + 36, Ti, Tj, flip != 0, loss_kind, loss_scale, lin, out + 1);
    else out[0] = pg_edge_lin(PRIOR_RELATIVE, rec, rec + 12, rec + 24, rec + 36, Ti, Tj, flip != 0, loss_kind, loss_scale, lin, out + 1);
}

void pgc_cost(int kind, const double *rec, const double *Ti, const double *Tj, int loss_kind, double loss_scale, double *out)
{
    out[0] = pg_edge_cost(kind, rec, rec + 12, rec + 24, rec + 36, Ti, Tj, loss_kind, loss_scale, out + 1);
}

void pgc_retract(const double *x, const double *d, double *out) { retract_pose(x, d, out); }

}
