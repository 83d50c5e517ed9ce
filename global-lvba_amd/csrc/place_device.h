// place_device.h -- scan-descriptor place recognition (lvba_place_*): the scalar arithmetic of the rule -- the bin of a point, the
// ring key, the normalised columns, the shift distance, the lexicographic orders and the selection.  Also compiles as plain C++
// (tests/place_check.cpp).  The including file is built without floating-point contraction: the bin of a point and every
// comparison of two distances are discrete decisions.  include/lvba_hip.h has the definitions; DESIGN.md §10e the rationale.
//   D [Nr][Ns] fp32   the descriptor: per (ring, sector) cell the largest (float)(z + z_offset) of its points, at least 0
//   key [Nr] fp32     key[ring] = (float)((double)(number of sectors with D > 0) / Ns)
//   U [Nr][Ns] fp64   ring-major; column j is D[:, j] / |D[:, j]|, the sum of squares in ring order; a zero column stays zero
//   mask [2] u64      bit j set iff column j is not empty (Ns <= 128)
// The gap clause and the (value, index) order are loop_device.h's: loop_gap_ok, loop_less (a float promotes exactly).
#pragma once
#include <math.h>
#include <stdint.h>
#include "loop_device.h"

namespace lvba {

constexpr int PLACE_MAX_RINGS = 32, PLACE_MAX_SECTORS = 128, PLACE_MAX_K = 32; // n_rings, n_sectors, n_key_candidates
constexpr double PLACE_PI = 3.14159265358979323846;

struct PlaceParams { // lvba_place_opts on the device
    int32_t n_rings, n_sectors, submap_size, min_gap, n_key, max_per_frame, query_stride;
    double min_range, max_range, z_offset, max_distance;
};

struct PlaceKey { // a (key distance, frame) pair, ordered lexicographically
    float d2;
    int32_t idx;
};

// The cell ring * Ns + sector of a body-frame point and its value *h, or -1: outside [min_range, max_range), not finite, or
// with a value that cannot raise a cell above its floor of 0.
LVBA_HD int place_bin(float xf, float yf, float zf, const PlaceParams &p, float *h)
{
    const double x = xf, y = yf, z = zf;
    const double r = sqrt(x * x + y * y);
    if (!(r >= p.min_range && r < p.max_range)) return -1; // also NaN and inf
    const float hv = (float)(z + p.z_offset);
    if (!(hv > 0.0f && hv < INFINITY)) return -1;
    int ring = (int)floor(r * (double)p.n_rings / p.max_range);
    if (ring > p.n_rings - 1) ring = p.n_rings - 1;
    int sector = (int)floor((atan2(y, x) + PLACE_PI) * (double)p.n_sectors / (2.0 * PLACE_PI));
    if (sector > p.n_sectors - 1) sector = p.n_sectors - 1;
    *h = hv;
    return ring * p.n_sectors + sector;
}

// key[ring] of a descriptor row (stride 1 between sectors)
LVBA_HD float place_ring_key(const float *row, int ns)
{
    int c = 0;
    for (int j = 0; j < ns; ++j) c += row[j] > 0.0f ? 1 : 0;
    return (float)((double)c / (double)ns);
}

// Column j of D (element stride ns between rings) normalised into column j of U; returns whether the column is not empty.
LVBA_HD bool place_column(const float *D, int nr, int ns, int j, double *U)
{
    double s = 0.0;
    for (int r = 0; r < nr; ++r) {
        const double d = D[r * ns + j];
        s = s + d * d;
    }
    const double norm = sqrt(s);
    for (int r = 0; r < nr; ++r) U[r * ns + j] = norm > 0.0 ? (double)D[r * ns + j] / norm : 0.0;
    return norm > 0.0;
}

LVBA_HD float place_key_d2(const float *kq, const float *kf, int nr)
{
    float acc = 0.0f;
    for (int r = 0; r < nr; ++r) {
        const float d = kq[r] - kf[r];
        acc = acc + d * d;
    }
    return acc;
}

// Keep the k smallest (d2, f) pairs seen so far in top[0 .. *n), ascending.
LVBA_HD void place_keep(PlaceKey *top, int *n, int k, float d2, int32_t f)
{
    int p = *n;
    if (p == k) {
        if (!loop_less(d2, f, top[k - 1].d2, top[k - 1].idx)) return;
        p = k - 1;
    } else {
        *n = p + 1;
    }
    while (p > 0 && loop_less(d2, f, top[p - 1].d2, top[p - 1].idx)) {
        top[p] = top[p - 1];
        --p;
    }
    top[p].d2 = d2; top[p].idx = f;
}

LVBA_HD bool place_bit(const uint64_t *m, int j) { return ((j < 64 ? m[0] : m[1]) >> (j & 63)) & 1; } // (no indexed register array)

// dist(s) of query q against frame c: 1 - sim(s) / n(s).  The sum runs over every column in (j, ring) order; a column that is
// empty on either side adds +0.0 terms to a sum that is never -0.0, which leaves the bits of the sum over the other columns.
LVBA_HD double place_dist_at(const double *Uq, const double *Uc, const uint64_t *mq, const uint64_t *mc, int nr, int ns, int s)
{
    double sim = 0.0;
    int n = 0;
    for (int j = 0; j < ns; ++j) {
        int jq = j - s;
        if (jq < 0) jq += ns;
        n += place_bit(mc, j) && place_bit(mq, jq) ? 1 : 0;
        for (int r = 0; r < nr; ++r) sim = sim + Uq[r * ns + jq] * Uc[r * ns + j];
    }
    return n > 0 ? 1.0 - sim / (double)n : 1.0;
}

// 2 pi shift / Ns wrapped to (-pi, pi]
LVBA_HD double place_yaw(int shift, int ns)
{
    const double y = 2.0 * PLACE_PI * (double)shift / (double)ns;
    return y > PLACE_PI ? y - 2.0 * PLACE_PI : y;
}

// The selection among a query's K picked frames f[k] (-1: none) with distances dist[k], in three steps of one pass each.
// 1: pick k is its submap's ref -- no other pick of the submap has a smaller (dist, f) -- and within max_distance
LVBA_HD bool place_eligible(int k, int K, const int32_t *f, const double *dist, int S, double max_distance)
{
    if (f[k] < 0 || !(dist[k] <= max_distance)) return false;
    for (int a = 0; a < K; ++a)
        if (a != k && f[a] >= 0 && f[a] / S == f[k] / S && loop_less(dist[a], f[a], dist[k], f[k])) return false;
    return true;
}
// 2: fewer than max_per_frame eligible picks have a smaller (dist, w)
LVBA_HD bool place_kept(int k, int K, const int32_t *f, const double *dist, const uint8_t *eligible, int S, int max_per_frame)
{
    if (!eligible[k]) return false;
    int before = 0;
    for (int a = 0; a < K; ++a)
        if (a != k && eligible[a] && loop_less(dist[a], f[a] / S, dist[k], f[k] / S)) ++before;
    return before < max_per_frame;
}
// 3: the place of a kept pick in the query's output: the number of kept picks of a lower submap
LVBA_HD int place_slot(int k, int K, const int32_t *f, const uint8_t *kept, int S)
{
    int slot = 0;
    for (int a = 0; a < K; ++a)
        if (kept[a] && f[a] / S < f[k] / S) ++slot;
    return slot;
}

} // namespace lvba
