// Compile/link check of the pose-prior part of include/lvba_adapter.hpp (prior_pose / prior_position / prior_relative, the
// damping_iter_hip and lidar_ba overloads that take priors) against stand-ins for the reference's Eigen-based types.
// Returns 0 if the priors are packed right and (without a GPU) the library refuses loudly, or (with one) refines with them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/lvba_adapter.hpp"

struct Mat3 { double m[9]; double &operator()(int r, int c) { return m[3 * r + c]; } double operator()(int r, int c) const { return m[3 * r + c]; } };
struct PointCluster { Mat3 P; double v[3]; int N; };
struct IMUST { Mat3 R; double p[3]; };
struct PointXYZINormal { float x, y, z, pad0, nx, ny, nz, pad1, intensity, curvature, pad2, pad3; };
struct Cloud { std::vector<PointXYZINormal> points; };
struct VOX_HESS { int win_size; std::vector<const std::vector<PointCluster> *> plvec_voxels; };

static IMUST ident(double px)
{
    IMUST s;
    std::memset(&s, 0, sizeof s);
    s.R(0, 0) = s.R(1, 1) = s.R(2, 2) = 1;
    s.p[0] = px;
    return s;
}

int main()
{
    // packing
    const IMUST T = ident(0.5);
    const lvba_prior a = lvba::prior_pose(0, T, 0.01, 0.1);
    if (a.kind != LVBA_PRIOR_POSE || a.i != 0 || a.meas[0] != 1.0 || a.meas[9] != 0.5 || a.sqrt_info[0] != 100.0 || a.sqrt_info[35] != 10.0 ||
        a.offset_i[0] != 0.0)
        return 1;
    const double z[3] = {1, 2, 3}, arm[3] = {0.1, 0.0, 1.2};
    const lvba_prior b = lvba::prior_position(2, z, 0.05, arm);
    if (b.kind != LVBA_PRIOR_POSITION || b.i != 2 || b.meas[11] != 3.0 || b.sqrt_info[0] != 20.0 || b.sqrt_info[7] != 20.0 ||
        b.sqrt_info[14] != 20.0 || b.offset_i[0] != 1.0 || b.offset_i[11] != 1.2)
        return 2;
    double L[36] = {};
    for (int k = 0; k < 6; ++k) L[7 * k] = 3.0;
    const lvba_prior c = lvba::prior_relative(0, 2, T, L);
    if (c.kind != LVBA_PRIOR_RELATIVE || c.i != 0 || c.j != 2 || c.sqrt_info[28] != 3.0 || c.meas[9] != 0.5) return 3;

    // damping_iter_hip with priors: a stiff POSE prior holds pose 0
    const int N = 3;
    std::vector<PointCluster> va(N), vb(N);
    for (auto *vv : {&va, &vb})
        for (auto &q : *vv) std::memset(&q, 0, sizeof q);
    const double pts[4][3] = {{1, 0, 0.01}, {0, 1, -0.01}, {-1, 0, 0.0}, {0, -1, 0.02}};
    auto push = [&](PointCluster &q, double ox) {
        for (auto &p : pts) {
            const double w[3] = {p[0] + ox, p[1], p[2]};
            for (int r = 0; r < 3; ++r) { q.v[r] += w[r]; for (int s = 0; s < 3; ++s) q.P(r, s) += w[r] * w[s]; }
            q.N++;
        }
    };
    push(va[0], 0.0); push(va[2], 0.1); push(vb[1], 0.0); push(vb[2], 0.2);
    VOX_HESS vh{N, {&va, &vb}};
    std::vector<IMUST> x{ident(0.0), ident(0.01), ident(-0.02)};
    x[0].p[2] = 0.03;
    const IMUST x0 = x[0];
    try {
        std::vector<lvba_prior> pri{lvba::prior_pose(0, x0, 1e-7, 1e-7), lvba::prior_relative(1, 2, ident(-0.03), 0.01, 0.01)};
        const auto tr = lvba::damping_iter_hip(x, vh, pri);
        double d = 0.0;
        for (int k = 0; k < 9; ++k) d = std::fmax(d, std::fabs(x[0].R.m[k] - x0.R.m[k]));
        for (int k = 0; k < 3; ++k) d = std::fmax(d, std::fabs(x[0].p[k] - x0.p[k]));
        std::printf("refined on the GPU with priors: %zu iterations, pose 0 moved %.3g\n", tr.size(), d);
        if (tr.empty() || d > 1e-9) return 4;
    } catch (const std::exception &e) {
        std::printf("refused: %s\n", e.what());
        if (!(lvba_device_count() == 0 && std::strstr(e.what(), "no CPU fallback"))) return 5;
    }

    // the LiDAR stage with frame priors: two windows of one frame pair each, a position fix on every frame
    Cloud c0, c1;
    for (int i = 0; i < 40; ++i) {
        PointXYZINormal p{};
        p.x = 0.1f + 0.02f * (i % 8); p.y = 0.1f + 0.1f * (i / 8); p.z = 0.5f + 0.001f * ((i * 7) % 3);
        p.intensity = 100.f;
        (i % 2 ? c1 : c0).points.push_back(p);
    }
    try {
        std::vector<const Cloud *> four{&c0, &c1, &c0, &c1};
        std::vector<IMUST> x4(4, ident(0.0));
        lvba_lidar_ba_opts lo;
        lvba_lidar_ba_default_opts(&lo);
        lo.window.window_size = 2;
        lo.window.voxel.voxel_size = 1.0; lo.stage_voxel_size[0] = lo.stage_voxel_size[1] = 1.0;
        const double zero[3] = {0, 0, 0};
        std::vector<lvba_prior> fp;
        for (int f = 0; f < 4; ++f) fp.push_back(lvba::prior_position(f, zero, 0.01));
        fp.push_back(lvba::prior_relative(0, 1, ident(0.0), 0.01, 0.01)); // one anchor: dropped
        int32_t used = -1, dropped = -1;
        const auto rep = lvba::lidar_ba(four, x4, lo, fp, 0, &used, &dropped);
        std::printf("lidar_ba with frame priors on the GPU: %d anchors, %d priors used, %d dropped\n", rep.n_anchors, used, dropped);
        if (rep.n_frames != 4 || used + dropped != 5 || dropped < 1) return 6;
    } catch (const std::exception &e) {
        std::printf("refused: %s\n", e.what());
        if (!(lvba_device_count() == 0 && std::strstr(e.what(), "no CPU fallback"))) return 7;
    }
    return 0;
}
