// undistort_check.cpp -- csrc/undistort_device.h compiled for the host (tests/test_undistort_host.py): the position of every target
// pixel, and the images walked the way undistort_kernel walks them -- a lane's four pixels through und_pixel, packed by und_pack
// into three dwords, the bytes taken out of the dwords again.  TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include "../global-lvba_amd/csrc/undistort_device.h"
#include "../include/lvba_hip.h"

using namespace lvba;

extern "C" {

int emul_opts_size() { return (int)sizeof(lvba_undistort_opts); }

void emul_tile(int32_t *t) { t[0] = UND_PIXELS; t[1] = UND_TILE_W; t[2] = UND_TILE_H; t[3] = UND_BLOCK; }

// pin = fx' fy' cx' cy'; uv [ho][wo][2] (NaN where invalid), mask [ho][wo]
void emul_map(const double *intr, int w, int h, const double *pin, int wo, int ho, double *uv, uint8_t *mask)
{
    const TrkIntr cam = trk_intr_of(intr);
    const UndPinhole p{pin[0], pin[1], pin[2], pin[3]};
    for (int j = 0; j < ho; ++j)
        for (int i = 0; i < wo; ++i) {
            double u, v;
            const bool ok = und_locate(cam, p, w, h, i, j, u, v);
            const int64_t q = (int64_t)j * wo + i;
            uv[2 * q] = ok ? u : (double)NAN; uv[2 * q + 1] = ok ? v : (double)NAN;
            mask[q] = ok ? 255 : 0;
        }
}

// bgr [m][h][w][3] -> out [m][ho][wo][3]; gains [m][3][2] or null
void emul_images(const double *intr, int w, int h, const double *pin, int wo, int ho, int border, int m, const uint8_t *bgr,
                 const int64_t *gains, uint8_t *out)
{
    const TrkIntr cam = trk_intr_of(intr);
    const UndPinhole p{pin[0], pin[1], pin[2], pin[3]};
    for (int b = 0; b < m; ++b) {
        const uint8_t *img = bgr + 3 * (int64_t)b * w * h;
        for (int j = 0; j < ho; ++j)
            for (int i0 = 0; i0 < wo; i0 += UND_PIXELS) {
                const int npx = wo - i0 < UND_PIXELS ? wo - i0 : UND_PIXELS;
                uint32_t px[UND_PIXELS] = {0, 0, 0, 0}, d[3];
                for (int q = 0; q < npx; ++q)
                    und_pixel(cam, p, w, h, i0 + q, j, (uint32_t)border, gains ? gains + 6 * (int64_t)b : nullptr,
                              [&](int y, int x) { return photo_texel_of(img + 3 * ((int64_t)y * w + x)); }, px[q]);
                und_pack(px, d);
                uint8_t *o = out + 3 * ((int64_t)b * wo * ho + (int64_t)j * wo + i0);
                for (int q = 0; q < 3 * npx; ++q) o[q] = (uint8_t)((d[q >> 2] >> (8 * (q & 3))) & 255u);
            }
    }
}

} // extern "C"
