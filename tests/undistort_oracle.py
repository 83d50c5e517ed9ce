"""numpy restatement of the undistorted-image rule (include/lvba_hip.h, "the undistorted images of the COLMAP export"; DESIGN.md
§10s).

The rule, once more.  Source camera intr = fx fy cx cy k1 k2 p1 p2, size w x h; target pinhole fx' fy' cx' cy', size w' x h'.
Target pixel (column i, row j): x = (i - cx') / fx', y = (j - cy') / fy'; r2 = x x + y y, r4 = r2 r2, radial = (1 + k1 r2) + k2 r4,
xd = x radial + ((2 p1) x y + p2 (r2 + 2 x x)), yd = y radial + (p1 (r2 + 2 y y) + (2 p2) x y), u = fx xd + cx, v = fy yd + cy,
every operation one rounded fp64 operation in this order.  Valid iff everything is finite and 0 <= u < w - 1, 0 <= v < h - 1.
X = floor(u), a = floor((u - X) 256), likewise Y, b; the four texels weigh (256 - a)(256 - b), a (256 - b), (256 - a) b, a b; per
channel c = sum weight byte, c16 = (c + 128) >> 8; with gains c16 = clip((A c16 + B + 32768) // 65536, 0, 65280); the byte is
(c16 + 128) >> 8.  An invalid pixel is `border`, its mask byte 0; a valid one's is 255.

The vectorised functions and the plain loops at the end (tiny cases only) are written independently of one another."""
import math

import numpy as np

ONE, C_MAX = 65536, 65280


def resolve(intr, width, height, fx=0.0, fy=0.0, cx=0.0, cy=0.0, out_width=0, out_height=0, border=0, **_):
    """(pinhole (fx', fy', cx', cy'), (w', h'), border) of the options: fx = 0 takes all four from the source, a size of 0 the source's"""
    pin = tuple(float(v) for v in intr[:4]) if fx == 0 else (float(fx), float(fy), float(cx), float(cy))
    return pin, (int(out_width) or int(width), int(out_height) or int(height)), int(border)


def position(intr, width, height, **opts):
    """(uv float64 [h', w', 2], NaN where invalid; mask uint8 [h', w'])"""
    (fxp, fyp, cxp, cyp), (wo, ho), _ = resolve(intr, width, height, **opts)
    fx, fy, cx, cy, k1, k2, p1, p2 = (np.float64(v) for v in intr)
    i, j = np.meshgrid(np.arange(wo, dtype=np.float64), np.arange(ho, dtype=np.float64))
    with np.errstate(all="ignore"):
        x, y = (i - np.float64(cxp)) / np.float64(fxp), (j - np.float64(cyp)) / np.float64(fyp)
        r2 = x * x + y * y
        r4 = r2 * r2
        radial = 1.0 + k1 * r2 + k2 * r4
        xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
        yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
        u, v = fx * xd + cx, fy * yd + cy
        ok = np.isfinite(xd) & np.isfinite(yd) & np.isfinite(u) & np.isfinite(v)
        ok &= (u >= 0.0) & (u < float(width - 1)) & (v >= 0.0) & (v < float(height - 1))
    uv = np.stack([np.where(ok, u, np.nan), np.where(ok, v, np.nan)], -1)
    return uv, np.where(ok, 255, 0).astype(np.uint8)


def images(bgr, intr, gains=None, **opts):
    """uint8 [m, h', w', 3] of bgr uint8 [m, h, w, 3]; gains None or int64 [m, 3, 2]"""
    bgr = np.asarray(bgr, np.uint8)
    m, h, w = bgr.shape[:3]
    uv, mask = position(intr, w, h, **opts)
    border = resolve(intr, w, h, **opts)[2]
    ok = mask != 0
    u, v = np.where(ok, uv[..., 0], 0.0), np.where(ok, uv[..., 1], 0.0)
    xf, yf = np.floor(u), np.floor(v)
    a, b = np.floor((u - xf) * 256.0).astype(np.int64), np.floor((v - yf) * 256.0).astype(np.int64)
    x, y = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x + 1, w - 1), np.minimum(y + 1, h - 1)      # (only the invalid pixels' dummies are clamped)
    out = np.zeros((m,) + mask.shape + (3,), np.uint8)
    for q in range(m):
        img = bgr[q].astype(np.int64)
        c = ((256 - a) * (256 - b))[..., None] * img[y, x] + (a * (256 - b))[..., None] * img[y, x1] + \
            ((256 - a) * b)[..., None] * img[y1, x] + (a * b)[..., None] * img[y1, x1]
        c16 = (c + 128) >> 8
        if gains is not None:
            g = np.asarray(gains, np.int64)[q]
            c16 = np.clip((g[:, 0] * c16 + g[:, 1] + 32768) // ONE, 0, C_MAX)
        out[q] = np.where(ok[..., None], (c16 + 128) >> 8, border).astype(np.uint8)
    return out


# ---- the rule as plain loops (tiny cases only), on Python floats and integers
def loops(bgr, intr, gains=None, **opts):
    """(uv, mask, out) as nested lists"""
    m, h, w = np.asarray(bgr).shape[:3]
    (fxp, fyp, cxp, cyp), (wo, ho), border = resolve(intr, w, h, **opts)
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(v) for v in intr)
    uv = [[None] * wo for _ in range(ho)]
    mask = [[0] * wo for _ in range(ho)]
    out = [[[[border] * 3 for _ in range(wo)] for _ in range(ho)] for _ in range(m)]
    for j in range(ho):
        for i in range(wo):
            x, y = (float(i) - cxp) / fxp, (float(j) - cyp) / fyp
            r2 = x * x + y * y
            r4 = r2 * r2
            radial = 1.0 + k1 * r2 + k2 * r4
            xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
            yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
            u, v = fx * xd + cx, fy * yd + cy
            if not (all(math.isfinite(t) for t in (xd, yd, u, v)) and 0.0 <= u < w - 1 and 0.0 <= v < h - 1):
                continue
            uv[j][i], mask[j][i] = (u, v), 255
            X, Y = int(math.floor(u)), int(math.floor(v))
            a, b = int(math.floor((u - X) * 256.0)), int(math.floor((v - Y) * 256.0))
            for q in range(m):
                for k in range(3):
                    c = (256 - a) * (256 - b) * int(bgr[q][Y][X][k]) + a * (256 - b) * int(bgr[q][Y][X + 1][k]) + \
                        (256 - a) * b * int(bgr[q][Y + 1][X][k]) + a * b * int(bgr[q][Y + 1][X + 1][k])
                    c16 = (c + 128) >> 8
                    if gains is not None:
                        c16 = min(max((int(gains[q][k][0]) * c16 + int(gains[q][k][1]) + 32768) // ONE, 0), C_MAX)
                    out[q][j][i][k] = (c16 + 128) >> 8
    return uv, mask, out
