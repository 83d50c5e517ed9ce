// image_set.hip -- the resident key-point table of the image front ends (image_set.h): upload, undistortion, release.
// Built without floating-point contraction (build.py): trk_undistort rounds expression by expression, as the reference does.
#include <math.h>
#include "image_set.h"
#include "mempool.h"

namespace lvba {

// a thread per key point: trk_undistort, NaN where it fails (once per lvba_match_set_geometry and per lvba_verify_create)
static __global__ __launch_bounds__(256) void image_set_undistort_kernel(int64_t n, const float *__restrict__ uv, const TrkIntr cam, double *__restrict__ xy)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double x, y;
    if (!trk_undistort(cam, (double)uv[2 * i], (double)uv[2 * i + 1], x, y)) x = y = NAN;
    xy[2 * i] = x; xy[2 * i + 1] = y;
}

int32_t image_set_upload(ImageSet &t, bool offsets, const float *uv)
{
    const size_t total = (size_t)t.off.back();
    if (offsets && !t.d_off) {
        HIPCHK(pool_alloc(&t.d_off, t.off.size())); HIPCHK(copy_h2d(t.d_off, t.off.data(), 8 * t.off.size()));
    }
    if (uv && total > 0) {
        if (!t.d_uv) HIPCHK(pool_alloc(&t.d_uv, 2 * total));
        HIPCHK(copy_h2d(t.d_uv, uv, 8 * total));
    }
    return LVBA_OK;
}

int32_t image_set_undistort(ImageSet &t, const TrkIntr &cam, const float *uv, bool keep_uv)
{
    const size_t total = (size_t)t.off.back();
    if (total == 0) return LVBA_OK;
    ScopedStream sg;
    HIPCHK(sg.acquire());
    DevArr<float> tmp(sg.s);
    if (keep_uv) TRY(image_set_upload(t, false, uv));
    else { HIPCHK(tmp.alloc(2 * total)); HIPCHK(tmp.upload(uv, 2 * total)); }
    if (!t.d_xy) HIPCHK(pool_alloc(&t.d_xy, 2 * total));
    image_set_undistort_kernel<<<(unsigned)((total + 255) / 256), 256, 0, sg.s>>>((int64_t)total, keep_uv ? t.d_uv : tmp, cam, t.d_xy);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sg.s));
    return LVBA_OK;
}

void image_set_free(ImageSet &t)
{
    for (void *p : {(void *)t.d_off, (void *)t.d_uv, (void *)t.d_xy})
        if (p) DevicePool::get().free(p);
}

} // namespace lvba
