// map_quality_device.h -- the per-point rules of the map-quality metrics (map_quality.hip) as host/device-neutral functions, so
// that the very code the kernels run is also compiled for the CPU (tests/mapq_check.cpp, tests/test_mapq_host.py).
//   cell index     floor(w / edge) per axis, edge = radius (1 + 2^-20): STRICTLY larger than the radius.  Two points whose
//                  coordinates differ by at most the radius then differ by at most 1 - 2^-20 in w / edge; the two quotients
//                  round by at most 2^-33 each (|w / edge| < 2^20), so their floors differ by at most one and the +-1 cell
//                  search cannot miss a neighbour.  With edge = radius, points exactly one radius apart can land two cells apart.
//   membership     d = (double)w_j - (double)w_k (exact), d2 = (dx dx + dy dy) + dz dz, d2 <= radius radius, inclusive
//   moments        count, sum d, sum d d^T about the query, in candidate order
//   finish         S = sum d d^T / n - m m^T; cyclic Jacobi with IEEE divisions (balm_math.h eig3, which gives the small
//                  eigenvalue of a near-planar neighbourhood to high relative accuracy); det S = lam0 lam1 lam2
// Files that include this one are built with -ffp-contract=off (build.py NO_CONTRACT): every expression rounds as written.
#pragma once
#include <math.h>
#include <stdint.h>
#include "balm_math.h"
#include "scan_points.h"

namespace lvba {

constexpr int MAPQ_CELL_LIMIT = KEY_BIAS - 1;      // |cell| < this: the neighbour cells c +- 1 stay packable (pack_key, scan_points.h)

LVBA_HD double mapq_cell_edge(double radius) { return radius * (1.0 + 1.0 / 1048576.0); }
LVBA_HD bool mapq_finite(const float w[3]) { return isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]); }
// cell of a finite point; false when a component is out of range
LVBA_HD bool mapq_cell_of(const float w[3], double edge, int64_t c[3])
{
    bool ok = true;
    for (int j = 0; j < 3; ++j) {
        const double q = floor((double)w[j] / edge);
        ok = ok && (fabs(q) < (double)MAPQ_CELL_LIMIT);
        c[j] = ok ? (int64_t)q : 0;
    }
    return ok;
}
// pack_key (scan_points.h) of a cell, under the name tests/mapq_check.cpp binds; new code calls pack_key
LVBA_HD uint64_t mapq_pack(int64_t x, int64_t y, int64_t z)
{
    const int64_t c[3] = {x, y, z};
    return pack_key(c);
}

struct MapqAcc {
    int32_t n;
    double s[3]; // sum d
    double q[6]; // sum d d^T: xx xy xz yy yz zz
};
LVBA_HD void mapq_clear(MapqAcc &a)
{
    a.n = 0;
    a.s[0] = a.s[1] = a.s[2] = 0.0;
    a.q[0] = a.q[1] = a.q[2] = a.q[3] = a.q[4] = a.q[5] = 0.0;
}
// one candidate c against the query wq (both widened to double), r2 = radius * radius
LVBA_HD void mapq_visit(MapqAcc &a, const double wq[3], double cx, double cy, double cz, double r2)
{
    const double dx = cx - wq[0], dy = cy - wq[1], dz = cz - wq[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 <= r2) {
        a.n += 1;
        a.s[0] += dx; a.s[1] += dy; a.s[2] += dz;
        a.q[0] += dx * dx; a.q[1] += dx * dy; a.q[2] += dx * dz;
        a.q[3] += dy * dy; a.q[4] += dy * dz; a.q[5] += dz * dz;
    }
}

struct MapqOut {
    int valid;
    double entropy, plane_var;
    float normal[3];
};
LVBA_HD void mapq_finish(const MapqAcc &a, int min_neighbors, MapqOut &o)
{
    o.valid = 0;
    o.entropy = o.plane_var = NAN;
    o.normal[0] = o.normal[1] = o.normal[2] = NAN;
    if (a.n < min_neighbors || a.n < 1) return;
    const double inv = 1.0 / (double)a.n;
    const double m0 = a.s[0] * inv, m1 = a.s[1] * inv, m2 = a.s[2] * inv;
    const double C[6] = {a.q[0] * inv - m0 * m0, a.q[1] * inv - m0 * m1, a.q[2] * inv - m0 * m2,
                         a.q[3] * inv - m1 * m1, a.q[4] * inv - m1 * m2, a.q[5] * inv - m2 * m2};
    double lam[3], U[9];
    eig3<true, false>(C, lam, U);
    const double det = lam[0] * lam[1] * lam[2];
    if (!(lam[0] > 0.0) || !(det > 0.0) || !isfinite(det)) return;
    const double two_pi_e = 2.0 * 3.14159265358979323846 * 2.71828182845904523536;
    o.valid = 1;
    o.entropy = 0.5 * log(two_pi_e * two_pi_e * two_pi_e * det);
    o.plane_var = lam[0];
    // the sign rule is applied to the stored (float) components: the first of the largest in magnitude is positive
    float n0 = (float)U[0], n1 = (float)U[3], n2 = (float)U[6];
    const float b0 = fabsf(n0), b1 = fabsf(n1), b2 = fabsf(n2);
    const float lead = (b0 >= b1 && b0 >= b2) ? n0 : (b1 >= b2 ? n1 : n2);
    if (lead < 0.f) { n0 = -n0; n1 = -n1; n2 = -n2; }
    o.normal[0] = n0; o.normal[1] = n1; o.normal[2] = n2;
}

} // namespace lvba
