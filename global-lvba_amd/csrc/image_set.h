// image_set.h -- what the image front ends (match.hip, verify.hip, track_graph.hip, covis.hip, resect.hip) share on the host: the resident
// key-point table of a set of images, and the argument checks of their entry points, one wording each; an entry point composes
// the checks it applies, in its own order.  The undistortion is image_set.hip, built without floating-point contraction; here
// is integer code, comparisons and copies only, so a translation unit that contracts (track_graph.hip) may include this.
#pragma once
#include <cmath>
#include <vector>
#include "lvba_common.h"
#include "tracks_device.h"

namespace lvba {

struct ImageSet {                // the key points of n_images images, image after image; the d_ members once asked for
    int device = 0;
    int32_t n_images = 0;
    std::vector<int64_t> off;   // [n_images + 1]; off.back() key points in all
    int64_t *d_off = nullptr;   // [n_images + 1]
    float *d_uv = nullptr;      // [total][2] pixels
    double *d_xy = nullptr;     // [total][2] undistorted normalised points, NaN where trk_undistort fails
};
// the offsets, if asked for and not yet resident (they never change); the pixels uv [total][2], if given (blocking copies)
int32_t image_set_upload(ImageSet &t, bool offsets, const float *uv);
// d_xy from the pixels uv [total][2] on the host, which go into the table (keep_uv) or stay on the device for this call only
int32_t image_set_undistort(ImageSet &t, const TrkIntr &cam, const float *uv, bool keep_uv);
void image_set_free(ImageSet &t); // the caller has set the device and drained it

// ---- argument checks: LVBA_OK, or LVBA_ERR_ARG through lvba_fail
// off [n + 1] starts at 0 and never decreases; no run is longer than max_run where that is >= 0.  `what` names a run ("image").
inline int32_t check_offsets(const char *name, const char *what, int64_t n, const int64_t *off, int64_t max_run = -1)
{
    if (off[0] != 0) return lvba_fail(LVBA_ERR_ARG, "%s[0] = %lld (0)", name, (long long)off[0]);
    for (int64_t i = 0; i < n; ++i) {
        const long long len = off[i + 1] - off[i];
        if (len < 0) return lvba_fail(LVBA_ERR_ARG, "%s decreases at %s %lld", name, what, (long long)i);
        if (max_run >= 0 && len > max_run)
            return lvba_fail(LVBA_ERR_ARG, "%s %lld has %lld entries in %s (at most %lld)", what, (long long)i, len, name, (long long)max_run);
    }
    return LVBA_OK;
}
inline int32_t check_intrinsics_finite(const double intr[8])
{
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(intr[k])) return lvba_fail(LVBA_ERR_ARG, "intrinsic %d is not finite", k);
    return LVBA_OK;
}
inline int32_t check_focal_lengths(const double intr[8])
{
    return intr[0] > 0.0 && intr[1] > 0.0 ? LVBA_OK : lvba_fail(LVBA_ERR_ARG, "focal lengths %g, %g (> 0)", intr[0], intr[1]);
}
// cameras [first, first + n) of v [.][per]: Rcw with per = 9 ("rotation"), tcw with per = 3 ("translation")
inline int32_t check_cameras_finite(const char *what, const double *v, int per, int64_t first, int64_t n)
{
    for (int64_t k = per * first; k < per * (first + n); ++k)
        if (!std::isfinite(v[k])) return lvba_fail(LVBA_ERR_ARG, "camera %lld: non-finite %s", (long long)(k / per), what);
    return LVBA_OK;
}
inline int32_t check_rotations_finite(const double *Rcw, int64_t first, int64_t n) { return check_cameras_finite("rotation", Rcw, 9, first, n); }
inline int32_t check_translations_finite(const double *tcw, int64_t first, int64_t n) { return check_cameras_finite("translation", tcw, 3, first, n); }
inline int32_t check_image_pair(int64_t a, int64_t b, int64_t n_images)
{
    const bool ok = a >= 0 && a < n_images && b >= 0 && b < n_images && a != b;
    return ok ? LVBA_OK : lvba_fail(LVBA_ERR_ARG, "pair (%lld, %lld): two different images of %lld", (long long)a, (long long)b, (long long)n_images);
}

} // namespace lvba
