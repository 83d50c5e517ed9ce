// tracks.hip -- per-track landmark initialisation on the device: one lane per feature track.
//
// Replaces the triangulation candidate of LvbaSystem::BuildTracksAndFuse3D (reference src/lvba_system.cpp:1110-1140):
//   TriangulateTrackDLT            src/lvba_system.cpp:50-111   A^T A of the DLT rows (undistorted normalised pixels), its
//                                                               smallest eigenvector, de-homogenisation
//   ComputeMeanReproj              src/lvba_system.cpp:8-48     mean pixel error of the candidate over the track
//   undistortPixelToNormalized, projectWorldToPixel             include/utils.hpp:168-233
// The 4x4 symmetric eigenproblem is solved by cyclic Jacobi rotations in registers (Eigen::SelfAdjointEigenSolver
// upstream); the reference walks an unordered_map, here observations are taken in the caller's order -- the sums differ
// at rounding level only.  The graph part of track building (BFS over matches, view-angle filter) stays with the caller.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "lvba_common.h"
#include "mempool.h"
#include "image_set.h"
#include "tracks_device.h"

using namespace lvba;

namespace {

typedef TrkIntr Intr;

__global__ void tri_kernel(int64_t n, const int64_t *__restrict__ obs_off, const int32_t *__restrict__ obs_cam,
                           const double *__restrict__ obs_uv, const double *__restrict__ Rcw, const double *__restrict__ tcw,
                           int32_t n_cams, Intr cam, double *__restrict__ Xout, double *__restrict__ err_out,
                           int32_t *__restrict__ cnt_out, uint8_t *__restrict__ ok_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double *Xo = Xout + 3 * i;
    Xo[0] = Xo[1] = Xo[2] = 0.0;
    err_out[i] = INFINITY;
    cnt_out[i] = 0;
    ok_out[i] = 0;
    const int64_t a = obs_off[i], b = obs_off[i + 1];
    double X[3] = {0.0, 0.0, 0.0}, mean;
    int cnt;
    const bool ok = trk_dlt(cam, Rcw, tcw, n_cams, a, (const int32_t *)nullptr, (int)(b - a), obs_cam, obs_uv, X, mean, cnt);
    Xo[0] = X[0]; Xo[1] = X[1]; Xo[2] = X[2];
    cnt_out[i] = cnt;
    err_out[i] = mean;
    ok_out[i] = ok ? 1 : 0;
}

} // namespace

extern "C" int32_t lvba_triangulate_tracks(int32_t device, int32_t n_cams, int64_t n_tracks, const int64_t *obs_off,
                                           const int32_t *obs_cam, const double *obs_uv, const double *Rcw, const double *tcw,
                                           const double intr[8], double *X, double *mean_reproj, int32_t *count, uint8_t *ok)
{
    if (n_cams < 1 || n_tracks < 0 || !obs_off || !Rcw || !tcw || !intr || !X || !mean_reproj || !count || !ok)
        return lvba_fail(LVBA_ERR_ARG, "null argument or n_cams < 1");
    if (n_tracks == 0) return LVBA_OK;
    TRY(check_offsets("obs_off", "track", n_tracks, obs_off)); // the kernel walks [obs_off[t], obs_off[t + 1]) of O-element arrays
    const int64_t O = obs_off[n_tracks];
    if (O > 0 && (!obs_cam || !obs_uv)) return lvba_fail(LVBA_ERR_ARG, "bad observation arrays");
    TRY(lvba::check_device(device));
    HIPCHK(hipSetDevice(device));
    ScopedStream sg;
    HIPCHK(sg.acquire());
    const hipStream_t s = sg.s;
    DevArr<int64_t> d_off(s); DevArr<int32_t> d_cam(s); DevArr<double> d_uv(s), d_R(s), d_t(s), d_X(s), d_err(s);
    DevArr<int32_t> d_cnt(s); DevArr<uint8_t> d_ok(s);
    HIPCHK(d_off.alloc((size_t)n_tracks + 1)); HIPCHK(d_cam.alloc((size_t)O)); HIPCHK(d_uv.alloc(2 * (size_t)O));
    HIPCHK(d_R.alloc(9 * (size_t)n_cams)); HIPCHK(d_t.alloc(3 * (size_t)n_cams));
    HIPCHK(d_X.alloc(3 * (size_t)n_tracks)); HIPCHK(d_err.alloc((size_t)n_tracks));
    HIPCHK(d_cnt.alloc((size_t)n_tracks)); HIPCHK(d_ok.alloc((size_t)n_tracks));
    HIPCHK(hipMemcpyAsync(d_off, obs_off, d_off.bytes((size_t)n_tracks + 1), hipMemcpyHostToDevice, s));
    if (O > 0) {
        HIPCHK(hipMemcpyAsync(d_cam, obs_cam, d_cam.bytes((size_t)O), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_uv, obs_uv, d_uv.bytes(2 * (size_t)O), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(d_R, Rcw, d_R.bytes(9 * (size_t)n_cams), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_t, tcw, d_t.bytes(3 * (size_t)n_cams), hipMemcpyHostToDevice, s));
    const Intr c = trk_intr_of(intr);
    tri_kernel<<<(unsigned)((n_tracks + 127) / 128), 128, 0, s>>>(n_tracks, d_off, d_cam, d_uv, d_R, d_t, n_cams, c, d_X, d_err,
                                                                  d_cnt, d_ok);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(X, d_X, d_X.bytes(3 * (size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(mean_reproj, d_err, d_err.bytes((size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(count, d_cnt, d_cnt.bytes((size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ok, d_ok, d_ok.bytes((size_t)n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return LVBA_OK;
}
