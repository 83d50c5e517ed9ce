// dynamic_device.h -- moving objects in the LiDAR map by range-image visibility (lvba_dynamic_*): the scalar arithmetic of the
// rule -- the cell of a body-frame point in a frame's range image, the dilated image, the body-frame query of a world point,
// the vote of one frame, the votes of a point over its window and the label.  Also compiles as plain C++
// (tests/dynamic_check.cpp).  The including file is built without floating-point contraction: the cell of a point and the two
// tolerance comparisons are discrete decisions.  include/lvba_hip.h has the definitions; DESIGN.md §10m the rationale.
//   I [n_rows][n_cols] fp32   per cell the smallest (float)r of the frame's points, +inf where there is none; built as the bits
//                             of non-negative floats, which order like the values
//   M [n_rows][n_cols] fp32   the minimum of I over the (2 halo + 1)^2 neighbourhood; rows clipped, columns wrap
#pragma once
#include <math.h>
#include <stdint.h>
#include "place_device.h" // PLACE_PI, LVBA_HD
#include "scan_points.h"

namespace lvba {

constexpr int DYN_MAX_ROWS = 1024, DYN_MAX_COLS = 4096, DYN_MAX_HALO = 3;
constexpr uint32_t DYN_EMPTY_BITS = 0x7F800000u; // +inf: a cell without a point
enum { DYN_NO_EVIDENCE = 0, DYN_FREE = 1, DYN_SUPPORT = 2 };

struct DynParams { // lvba_dynamic_opts on the device
    int32_t n_rows, n_cols, halo, window, min_free;
    double el_min, el_max, min_range, max_range, abs_tol, rel_tol, free_ratio;
};

// The cell row * n_cols + col of a body-frame point and its range *r, or -1: not finite, outside [min_range, max_range), on
// the sensor axis, or outside [el_min, el_max).
LVBA_HD int dyn_cell(double x, double y, double z, const DynParams &p, double *r)
{
    const double s = x * x + y * y;
    const double rho = sqrt(s), rr = sqrt(s + z * z);
    if (!(rr < INFINITY) || !(rr >= p.min_range && rr < p.max_range) || !(rho > 0.0)) return -1; // also NaN
    int col = (int)floor((atan2(y, x) + PLACE_PI) * (double)p.n_cols / (2.0 * PLACE_PI));
    if (col > p.n_cols - 1) col = p.n_cols - 1;
    const double e = atan2(z, rho);
    if (!(e >= p.el_min && e < p.el_max)) return -1;
    int row = (int)floor((e - p.el_min) * (double)p.n_rows / (p.el_max - p.el_min));
    if (row > p.n_rows - 1) row = p.n_rows - 1;
    *r = rr;
    return row * p.n_cols + col;
}

// M[row][col] of an image I (as floats or as their bits: both order alike)
template <class T> LVBA_HD T dyn_dilate(const T *I, int n_rows, int n_cols, int halo, int row, int col)
{
    T m = I[row * n_cols + col];
    for (int dr = -halo; dr <= halo; ++dr) {
        const int r = row + dr;
        if (r < 0 || r >= n_rows) continue;
        for (int dc = -halo; dc <= halo; ++dc) {
            int c = (col + dc) % n_cols;
            if (c < 0) c += n_cols;
            const T v = I[r * n_cols + c];
            if (v < m) m = v;
        }
    }
    return m;
}

// q = R_g^T (w - t_g): the world point w in the body frame of pose T_g, each component summed from left to right
LVBA_HD void dyn_to_body(const double *T, const double w[3], double q[3])
{
    const double d0 = w[0] - T[9], d1 = w[1] - T[10], d2 = w[2] - T[11];
    q[0] = T[0] * d0 + T[3] * d1 + T[6] * d2;
    q[1] = T[1] * d0 + T[4] * d1 + T[7] * d2;
    q[2] = T[2] * d0 + T[5] * d1 + T[8] * d2;
}

// what a frame whose dilated image reads m in the query's cell says about a query at range r_q
LVBA_HD int dyn_vote(float m, double r_q, const DynParams &p)
{
    if (!(m < INFINITY)) return DYN_NO_EVIDENCE;
    const double tol = p.abs_tol + p.rel_tol * r_q;
    if ((double)m > r_q + tol) return DYN_FREE;     // the frame saw through the point
    if ((double)m >= r_q - tol) return DYN_SUPPORT;
    return DYN_NO_EVIDENCE;                          // occluded
}

// the frames [*g0, *g1) that vote on the points of frame f of n
LVBA_HD void dyn_window(int f, int n, int window, int *g0, int *g1)
{
    *g0 = window <= 0 || f - window < 0 ? 0 : f - window;
    *g1 = window <= 0 || f + window + 1 > n ? n : f + window + 1;
}

// The votes on the world point w of frame f from the frames g of [ga, gb), g != f: poses [.][12] indexed by frame, M the dilated
// images of the frames from m_first on, `cells` floats each.
LVBA_HD void dyn_votes(const double w[3], int f, int ga, int gb, const double *poses, const float *M, int m_first, int64_t cells,
                       const DynParams &p, int32_t *n_free, int32_t *n_support)
{
    int32_t nf = 0, ns = 0;
    for (int g = ga; g < gb; ++g) {
        if (g == f) continue;
        double q[3], r_q;
        dyn_to_body(poses + 12 * (int64_t)g, w, q);
        const int c = dyn_cell(q[0], q[1], q[2], p, &r_q);
        if (c < 0) continue;
        const int v = dyn_vote(M[(int64_t)(g - m_first) * cells + c], r_q, p);
        nf += v == DYN_FREE ? 1 : 0;
        ns += v == DYN_SUPPORT ? 1 : 0;
    }
    *n_free += nf;
    *n_support += ns;
}

LVBA_HD uint8_t dyn_label(int32_t n_free, int32_t n_support, const DynParams &p)
{
    return n_free >= p.min_free && (double)n_free >= p.free_ratio * (double)(n_free + n_support) ? 1 : 0;
}

} // namespace lvba
