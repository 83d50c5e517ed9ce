// undistort_device.h -- scalar pieces of the undistorted-image export (undistort.hip; the rule is in include/lvba_hip.h,
// DESIGN.md §10s): where a pixel of the target pinhole image lies in the source image, and its three bytes.  Host/device-neutral,
// like photo_device.h; tests/undistort_check.cpp compiles it for the host.  The position is trk_project_cam on the pixel's viewing
// ray -- + - * / in fp64, in a file built without contraction --; everything after it is the fusion's integer arithmetic
// (photo_tap, photo_mix_channel) and the exposure stage's (expo_apply), none of them written a second time.
#pragma once
#include <math.h>
#include <stdint.h>
#include "photo_device.h"
#include "expo_device.h"

namespace lvba {

constexpr int UND_PIXELS = 4;                 // consecutive target pixels of a lane: twelve bytes, three dwords
constexpr int UND_TILE_W = 64, UND_TILE_H = 16; // target pixels of a workgroup: 16 lanes across, 16 rows -- 256 lanes
constexpr int UND_LANES_X = UND_TILE_W / UND_PIXELS;
constexpr int UND_BLOCK = UND_LANES_X * UND_TILE_H;
constexpr int UND_MAX_BATCH = 32768;          // images of a launch: the grid's third extent

struct UndPinhole { double fx, fy, cx, cy; }; // the target camera

// Where target pixel (column i, row j) is sampled in the w x h source: false where it is not (the projection fails, or (u, v)
// is outside photo_locate's range 0 <= u < w - 1, 0 <= v < h - 1).
LVBA_TRK_FN bool und_locate(const TrkIntr &cam, const UndPinhole &p, int w, int h, int i, int j, double &u, double &v)
{
    const double x = ((double)i - p.cx) / p.fx, y = ((double)j - p.cy) / p.fy;
    if (!trk_project_cam(cam, x, y, 1.0, u, v)) return false;
    return u >= 0.0 && u < (double)(w - 1) && v >= 0.0 && v < (double)(h - 1);
}

// the byte of a sample in units of 1/256 grey level: round half up; c16 <= 65280 gives at most 255
LVBA_TRK_FN uint32_t und_byte(int32_t c16) { return (uint32_t)((c16 + 128) >> 8); }

// The pixel as a word b | g << 8 | r << 16 (photo_texel_of's order), and whether it is valid; an invalid pixel is `border` in
// all three.  gains: null, or the image's [3][2].
template <class Texel>
LVBA_TRK_FN bool und_pixel(const TrkIntr &cam, const UndPinhole &p, int w, int h, int i, int j, uint32_t border,
                           const int64_t *__restrict__ gains, Texel texel, uint32_t &bgr)
{
    double u, v;
    if (!und_locate(cam, p, w, h, i, j, u, v)) { bgr = border | (border << 8) | (border << 16); return false; }
    const PhotoTap t = photo_tap(u, v, texel);
    bgr = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int32_t c16 = photo_mix_channel(t, k);
        if (gains) c16 = expo_apply(gains[2 * k], gains[2 * k + 1], c16);
        bgr |= und_byte(c16) << (8 * k);
    }
    return true;
}

// The twelve bytes of four pixel words as three little-endian dwords: byte q of the run is byte q & 3 of d [q >> 2].
LVBA_TRK_FN void und_pack(const uint32_t *__restrict__ px, uint32_t *__restrict__ d)
{
    d[0] = px[0] | (px[1] << 24);
    d[1] = (px[1] >> 8) | (px[2] << 16);
    d[2] = (px[2] >> 16) | (px[3] << 8);
}

} // namespace lvba
