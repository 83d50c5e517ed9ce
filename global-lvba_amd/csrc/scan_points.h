// scan_points.h -- what every front end does with a point of a scan set (points [P][3] fp32 + frame offsets) before anything
// else: the frame it belongs to, its frame's pose applied to it, the leaf key of down_sampling_voxel2, the 3 x 21-bit key
// packing.  Each rule is stated here once; voxelize.hip, window_ba.hip, fusion.hip, colorize.hip, map_quality.hip and
// register.hip (and, through their *_device.h headers, the host tests) call it.  Host/device-neutral, no HIP includes: also
// compiled by g++ (tests/scan_points_check.cpp).
// The functions are inline ON PURPOSE: the including translation unit's floating-point contraction setting applies to them
// (build.py: voxelize.hip contracts a*b+c into FMAs, the NO_CONTRACT files round every expression as written).  leaf_key_of
// is only exact as written without contraction: only NO_CONTRACT files may call it (an explicit -ffp-contract=fast overrides
// contraction pragmas, so nothing inside the function can protect it: voxelize.hip must not call it).
#pragma once
#include <math.h>
#include <stdint.h>
#include "segments.h"

#if defined(__HIPCC__)
#define LVBA_SP_HD __host__ __device__ __forceinline__
#else
#define LVBA_SP_HD inline
#endif

namespace lvba {

// The frame f of point i of a set, frame_off[f] - frame_off[0] <= i < frame_off[f + 1] - frame_off[0]: frame_off [n_frames + 1]
// may be a slice of a longer offset array (a window of the set, i counted from the window's first point) or start at 0.
// The search is segment_of (segments.h) over the offsets counted from the first.  n_frames >= 1 and
// 0 <= i < frame_off[n_frames] - frame_off[0].
LVBA_SP_HD int frame_of_point(const int64_t *__restrict__ frame_off, int n_frames, int64_t i)
{
    const int64_t base = frame_off[0];
    return segment_of([=](int f) { return frame_off[f] - base; }, n_frames, i);
}

// pose T = R (row-major) | t, 12 doubles: out = R p + t in double, each row summed from left to right
LVBA_SP_HD void pose_apply(const double *T, double x, double y, double z, double out[3])
{
    out[0] = T[0] * x + T[1] * y + T[2] * z + T[9];
    out[1] = T[3] * x + T[4] * y + T[5] * z + T[10];
    out[2] = T[6] * x + T[7] * y + T[8] * z + T[11];
}
// the same, stored as float (pl_transform, include/BALM/tools.hpp:385-395; src/lvba_system.cpp:1980-1987)
LVBA_SP_HD void pose_apply_f32(const double *T, double x, double y, double z, float out[3])
{
    double w[3];
    pose_apply(T, x, y, z, w);
    out[0] = (float)w[0]; out[1] = (float)w[1]; out[2] = (float)w[2];
}

// ---- voxel keys: three signed components in [-2^20, 2^20), biased and packed x << 42 | y << 21 | z ------------------------
constexpr int KEY_BIAS = 1 << 20;
LVBA_SP_HD uint64_t pack_key(const int64_t k[3])
{
    return ((uint64_t)(k[0] + KEY_BIAS) << 42) | ((uint64_t)(k[1] + KEY_BIAS) << 21) | (uint64_t)(k[2] + KEY_BIAS);
}

// down_sampling_voxel2 (tools.hpp:318-341) for a float point q and the double leaf: key = (int64)(float)(q / leaf), minus 1
// when negative (in float); d2 = squared distance to the leaf centre, dx*dx + dy*dy + dz*dz from left to right.  Returns
// false when a component falls outside the packable range (or q is not finite).
LVBA_SP_HD bool leaf_key_of(const float q[3], double leaf, int64_t k[3], double &d2)
{
    bool ok = true;
    double dd = 0.0;
    for (int j = 0; j < 3; ++j) {
        float loc = (float)((double)q[j] / leaf);
        if (loc < 0.f) loc -= 1.f;
        ok = ok && (fabsf(loc) < (float)KEY_BIAS);
        k[j] = ok ? (int64_t)loc : 0;
        const double c = ((double)k[j] + 0.5) * leaf;
        const double d = (double)q[j] - c;
        dd = dd + d * d;
    }
    d2 = dd;
    return ok;
}

} // namespace lvba
