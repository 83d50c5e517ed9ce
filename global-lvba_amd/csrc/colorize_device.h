// colorize_device.h -- the per-point rules of the LiDAR map colouriser (colorize.hip) as host/device-neutral functions, so that
// the very code the kernels run is also compiled for the CPU (tests/colorize_check.cpp, tests/test_colorize_host.py).
// Of the reference (src/lvba_system.cpp, LvbaSystem::VisualizeOptComparison, :1932-2144):
//   scan window           :1974       |t_scan - t_image| <= 0.5 (the difference is rounded first: not t0 <= t <= t1)
//   world point           :1980-1987  R p + t in double, stored as float (pose_apply_f32, scan_points.h)
//   projection            :2034-2045  projectWorldToPixel (include/utils.hpp:183-205), std::round, [0,W) x [0,H)
//   depth buffer          :2046-2058  replace when zc + 1e-6f < zbuf, zbuf = (float)zc; pixel kept when zbuf is finite
//   down_sampling_voxel2  include/BALM/tools.hpp:300-359 (key and squared distance to the leaf centre: leaf_key_of, scan_points.h)
// Files that include this one are built with -ffp-contract=off (build.py NO_CONTRACT): every expression rounds as written.
#pragma once
#include "tracks_device.h"
#include "scan_points.h"

namespace lvba {

// :1974 -- the image at t_img uses the scan at t_scan unless |t_scan - t_img| > half.  For ascending scan times the rounded
// difference is non-decreasing, so the scans used form one contiguous range (found by col_window_range).
LVBA_TRK_FN bool col_in_window(double t_scan, double t_img, double half) { return !(fabs(t_scan - t_img) > half); }
// [lo, hi): the scans of t[0..n) (ascending) inside the window of t_img
LVBA_TRK_FN void col_window_range(const double *t, int n, double t_img, double half, int &lo, int &hi)
{
    int a = 0, b = n; // first index with t - t_img >= -half
    while (a < b) {
        const int m = (a + b) >> 1;
        if (t[m] - t_img >= -half) b = m; else a = m + 1;
    }
    lo = a;
    b = n; // first index with t - t_img > half
    while (a < b) {
        const int m = (a + b) >> 1;
        if (t[m] - t_img > half) b = m; else a = m + 1;
    }
    hi = a;
}

// :1980-1987 -- the world point in double, stored as float; the leaf key of down_sampling_voxel2: the shared rules under the
// names tests/colorize_check.cpp binds.  New code calls pose_apply_f32 and leaf_key_of (scan_points.h).
LVBA_TRK_FN void col_world_point(const double *T, float x, float y, float z, float out[3]) { pose_apply_f32(T, x, y, z, out); }
LVBA_TRK_FN bool col_leaf_key(const float q[3], double leaf, int64_t k[3], double &d2) { return leaf_key_of(q, leaf, k, d2); }

// :2034-2045 -- projectWorldToPixel of the float point (widened back to double), std::round (half away from zero),
// bounds [0, W) x [0, H).  Returns false when the reference skips the point; else the row-major pixel and the depth zc.
LVBA_TRK_FN bool col_project(const TrkIntr &cam, const double *R, const double *t, const float pw[3], int W, int H, int64_t &pix,
                             double &zc)
{
    const double X[3] = {(double)pw[0], (double)pw[1], (double)pw[2]};
    const double X0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double X1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double Z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    double u, v;
    if (!trk_project_cam(cam, X0, X1, Z, u, v)) return false; // non-finite, Z <= 1e-12
    const double ru = round(u), rv = round(v);
    // static_cast<int> of anything this large is undefined upstream (x86-64 gives INT_MIN, out of bounds): skip it here
    if (!(fabs(ru) < 2.0e9 && fabs(rv) < 2.0e9)) return false;
    const int uu = (int)ru, vv = (int)rv;
    if (uu < 0 || uu >= W || vv < 0 || vv >= H) return false;
    pix = (int64_t)vv * W + uu;
    zc = Z;
    return true;
}

// :2046-2058 -- one step of the depth buffer: the point replaces the stored one when zc + 1e-6f < zbuf (in double, zbuf
// widened); zbuf then holds (float)zc.  Not a minimum: with the epsilon and the float store, the survivor is the end of a
// chain of first improvements in point order.
LVBA_TRK_FN bool col_depth_step(double zc, float &zbuf)
{
    const float eps = 1e-6f;
    if (zc + eps < zbuf) {
        zbuf = (float)zc;
        return true;
    }
    return false;
}
// The whole walk over one pixel's points, in point order: zc_at(q) = depth of the q-th of n.  Returns true when the pixel
// is kept (its final zbuf is finite, :2063-2067); winner = index q of the point stored last.
template <class ZAt>
LVBA_TRK_FN bool col_walk(int64_t n, ZAt zc_at, int64_t &winner)
{
    float zbuf = INFINITY;
    winner = -1;
    for (int64_t q = 0; q < n; ++q)
        if (col_depth_step(zc_at(q), zbuf)) winner = q;
    return winner >= 0 && isfinite(zbuf);
}

#if defined(__HIPCC__)
// One lane per point i of P points in frames frame_off[0 .. n_frames] (a slice of the set's offsets; pts points at its first
// point): the world point at the frame's pose, stored as float.  thin: a finite point whose leaf key cannot be packed sets *err.
// Shared by the coloured map (colorize.hip) and the map-quality metrics (map_quality.hip: thin = 0, err unused).
static __global__ void col_world_kernel(int64_t P, const float *__restrict__ pts, const int64_t *__restrict__ frame_off, int n_frames,
                                 const double *__restrict__ poses, double leaf, int thin, float *__restrict__ world,
                                 int *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float q[3];
    pose_apply_f32(poses + 12 * (int64_t)frame_of_point(frame_off, n_frames, i), pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], q);
    world[3 * i] = q[0]; world[3 * i + 1] = q[1]; world[3 * i + 2] = q[2];
    if (thin && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) { // only finite points can ever be projected
        int64_t k[3];
        double dd;
        if (!leaf_key_of(q, leaf, k, dd)) atomicOr(err, 1);
    }
}
#endif

} // namespace lvba
