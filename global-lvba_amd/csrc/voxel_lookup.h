// voxel_lookup.h -- the plane map's search tables and the world point -> plane association on them (src/lvba_system.cpp:1531-1565
// + findCorrespondPoint, bavoxel.hpp:320-333), shared by lvba_voxmap_find_planes (voxelize.hip) and the scan-to-map registration
// (register.hip).  Device code; the discrete decisions (root key, octants, table search) do not depend on the including file's
// floating-point contraction setting: the only product they add to is exact.
#pragma once
#include "voxel_internal.h"

namespace lvba {

enum : int { ST_NONE = 0, ST_DROP = 1, ST_PLANE = 2, ST_SPLIT = 3 };

// ---- shared per-point arithmetic (cut_voxel :809-815, root centre :826-829, cut_func :368-381) ------------------
__device__ __forceinline__ void octants_of(const double pw[3], const int64_t k[3], double vs, int &o1, int &o2)
{
    const float quater = (float)(vs / 4.0);
    o1 = 0; o2 = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float c0 = (float)((0.5 + (double)k[j]) * vs);
        const int b1 = pw[j] > (double)c0 ? 1 : 0;
        const float c1 = c0 + (float)(2 * b1 - 1) * quater;
        const int b2 = pw[j] > (double)c1 ? 1 : 0;
        o1 |= b1 << (2 - j);
        o2 |= b2 << (2 - j);
    }
}

// The searchable part of a map: R roots; per root its state and split bits, the mask of octant slots that hold a plane and the
// index of its first plane; per plane node centre (3) and normal (3).  A map of ONE window has its roots sorted by packed key
// (win_r0 = nullptr, n_windows = 1: the range to search is [0, R)).  A joint map of several windows (a submap set) holds a key
// once per window, window-major: window w's roots are [win_r0[w], win_r0[w + 1]) (device array of n_windows + 1 entries),
// sorted by key inside the range; plane indices stay those of the whole map.
struct VoxLookup {
    double vs = 0.0;
    int64_t R = 0;
    const uint64_t *root_key = nullptr, *mask = nullptr;
    const uint32_t *rootinfo = nullptr;
    const int32_t *plane_first = nullptr;
    const double *plane = nullptr;
    const int64_t *win_r0 = nullptr;
    int32_t n_windows = 1;
};

// The plane (unit normal n, offset d: n . x + d = 0) the world point pw falls on, among the roots [r0, r1) (a map of one
// window: [0, R)); false: none (no root, a dropped or empty octant, a degenerate normal, a non-finite or out-of-range point).
__device__ __forceinline__ bool vox_find_plane(const double pw[3], double vs, int64_t r0, int64_t r1, const uint64_t *__restrict__ root_key,
                                               const uint64_t *__restrict__ mask, const uint32_t *__restrict__ rootinfo,
                                               const int32_t *__restrict__ plane_first, const double *__restrict__ plane, double o[4])
{
    if (!(isfinite(pw[0]) && isfinite(pw[1]) && isfinite(pw[2]))) return false;
    int64_t k[3];
    if (!root_key_of(pw, vs, k)) return false;
    const uint64_t key = pack_key(k);
    int64_t lo = r0, hi = r1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (root_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo >= r1 || root_key[lo] != key) return false;
    const uint32_t info = rootinfo[lo];
    const int st0 = info & 0xff;
    int o1, o2;
    octants_of(pw, k, vs, o1, o2);
    int lane;
    if (st0 == ST_PLANE) lane = 0;
    else if (st0 == ST_SPLIT) lane = ((info >> (8 + o1)) & 1u) ? (o1 << 3 | o2) : (o1 << 3);
    else return false;
    const uint64_t m = mask[lo];
    if (!((m >> lane) & 1ull)) return false;
    const double *pl = plane + 6 * ((int64_t)plane_first[lo] + __popcll(lane ? (m & (~0ull >> (64 - lane))) : 0ull));
    const double nn = sqrt(pl[3] * pl[3] + pl[4] * pl[4] + pl[5] * pl[5]);
    if (!(isfinite(nn) && nn >= 1e-6 && isfinite(pl[0]) && isfinite(pl[1]) && isfinite(pl[2]))) return false;
    const double n0 = pl[3] / nn, n1 = pl[4] / nn, n2 = pl[5] / nn;
    o[0] = n0; o[1] = n1; o[2] = n2;
    o[3] = -(n0 * pl[0] + n1 * pl[1] + n2 * pl[2]);
    return true;
}

} // namespace lvba

struct lvba_voxmap_s;
// The tables of a map and its device and stream (voxelize.hip).  LVBA_ERR_UNSUPPORTED for a joint map of several windows or a
// view into one.  An empty map gives R = 0.
int32_t lvba_voxmap_lookup_tables(const lvba_voxmap_s *h, lvba::VoxLookup *out, int *device);
// The same for a submap set: a joint map of several windows comes with its window table (win_r0, n_windows); a map of one
// window is a set of one submap (win_r0 = nullptr).  LVBA_ERR_UNSUPPORTED for a view.
int32_t lvba_voxmap_lookup_tables_windows(const lvba_voxmap_s *h, lvba::VoxLookup *out, int *device);
