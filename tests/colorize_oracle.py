"""Plain restatement of the reference's LvbaSystem::VisualizeOptComparison (src/lvba_system.cpp:1932-2144) for ONE pose set,
the model the colouriser (lvba_colorize_*, csrc/colorize.hip) is held against.  TEST INFRASTRUCTURE ONLY.

    for image k:  scans with |t_scan - t_k| <= 0.5 (:1974), in scan order, their points in file order
                  world point = (float)(R p + t) in double (:1980-1987); skipped when the window holds no point (:1991-1996)
                  projectWorldToPixel of the float point, std::round, [0,W) x [0,H) (:2034-2045)
                  zbuf: replace when zc + 1e-6f < zbuf, zbuf = (float)zc (:2046-2058); colour = the pixel's b, g, r (:2051)
                  survivors in row-major pixel order (:2063-2067); images concatenated (:2069)
    down_sampling_voxel2(merged, leaf) (include/BALM/tools.hpp:300-359): per leaf voxel the first point at minimum d2

The projection is vectorised with numpy (elementwise IEEE operations in the reference's order, no fused multiply-add); the
depth buffer is walked point by point in Python.  The thinned cloud is returned sorted by leaf key (x, y, z), the order the
device emits; the reference's is unordered_map order."""
import numpy as np

EPS = float(np.float32(1e-6))
KEY_BIAS = 1 << 20


def world_points(cloud, T):
    """cloud [n,>=3] float32, T [12] = R row-major | t -> (float32)(R p + t) computed in double."""
    p = np.asarray(cloud, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T, np.float64).reshape(12)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[3 * r] * p[:, 0] + T[3 * r + 1] * p[:, 1]) + T[3 * r + 2] * p[:, 2]) + T[9 + r]).astype(np.float32)
    return out


def std_round(x):
    """std::round: half away from zero (np.round rounds half to even)."""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def project(pw, Rcw, tcw, intr, W, H):
    """projectWorldToPixel (include/utils.hpp:183-205) of float points pw [n,3] + the bounds of :2043-2045.
    Returns (ok [n] bool, pixel index [n] int64, zc [n] float64)."""
    X = np.asarray(pw, np.float32).astype(np.float64)
    R = np.asarray(Rcw, np.float64).reshape(3, 3)
    t = np.asarray(tcw, np.float64).reshape(3)
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(v) for v in np.asarray(intr, np.float64))
    Xc = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)]
    Z = Xc[2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(Xc[0]) & np.isfinite(Xc[1]) & np.isfinite(Z) & (Z > 1e-12)
        x, y = Xc[0] / Z, Xc[1] / Z
        r2 = x * x + y * y
        r4 = r2 * r2
        radial = (1.0 + k1 * r2) + k2 * r4
        xd = x * radial + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * x * x))
        yd = y * radial + (p1 * (r2 + 2.0 * y * y) + (2.0 * p2) * x * y)
        ok &= np.isfinite(xd) & np.isfinite(yd)
        u = fx * xd + cx
        v = fy * yd + cy
        ok &= np.isfinite(u) & np.isfinite(v)
        ru, rv = std_round(u), std_round(v)
        ok &= (np.abs(ru) < 2.0e9) & (np.abs(rv) < 2.0e9)
        uu = np.where(ok, ru, -1).astype(np.int64)
        vv = np.where(ok, rv, -1).astype(np.int64)
    ok &= (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
    return ok, np.where(ok, vv * W + uu, -1), Z


def depth_walk(zcs):
    """The depth buffer of one pixel over its points' zc in point order: (kept, index of the point stored last)."""
    zbuf, win = np.float32(np.inf), -1
    for q, zc in enumerate(zcs):
        if zc + EPS < float(zbuf):
            zbuf, win = np.float32(zc), q
    return bool(win >= 0 and np.isfinite(zbuf)), win


def colorize_image(pw, Rcw, tcw, intr, W, H, bgr):
    """One image: (xyz [s,3] float32, rgb [s,3] uint8) of the kept pixels in row-major order."""
    ok, pix, zc = project(pw, Rcw, tcw, intr, W, H)
    idx = np.nonzero(ok)[0]
    order = np.argsort(pix[idx], kind="stable")                      # each pixel's points, in point order
    idx = idx[order]
    pix_s = pix[idx]
    zl = zc[idx].tolist()
    starts = np.concatenate([[0], np.nonzero(np.diff(pix_s))[0] + 1, [len(idx)]]) if len(idx) else np.zeros(1, np.int64)
    sel, pixels = [], []
    for a, b in zip(starts[:-1], starts[1:]):
        kept, w = depth_walk(zl[a:b])
        if kept:
            sel.append(idx[a + w]); pixels.append(pix_s[a])
    sel, pixels = np.asarray(sel, np.int64), np.asarray(pixels, np.int64)
    img = np.asarray(bgr, np.uint8).reshape(H * W, 3)
    return pw[sel].astype(np.float32), img[pixels][:, ::-1].copy()


def leaf_keys(xyz, leaf):
    """down_sampling_voxel2's key (float quotient, minus 1 when negative) and d2 (tools.hpp:318-337)."""
    q = np.asarray(xyz, np.float32)
    loc = (q.astype(np.float64) / leaf).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32)
    k = loc.astype(np.int64)
    c = (k.astype(np.float64) + 0.5) * leaf
    d = q.astype(np.float64) - c
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return k, d2


def down_sampling_voxel2(xyz, rgb, leaf):
    """Per leaf voxel the first point (in merged order) at the smallest d2; sorted by key (x, y, z).  leaf < 0.001: unchanged."""
    if leaf < 0.001 or len(xyz) == 0:
        return xyz, rgb
    k, d2 = leaf_keys(xyz, leaf)
    pos = np.arange(len(xyz))
    order = np.lexsort((pos, d2, k[:, 2], k[:, 1], k[:, 0]))          # by key, then d2, then merged position
    ks = k[order]
    first = np.ones(len(order), bool)
    first[1:] = np.any(ks[1:] != ks[:-1], axis=1)
    keep = order[first]
    return xyz[keep], rgb[keep]


def colorize(clouds, scan_poses, scan_times, image_times, Rcw, tcw, intr, W, H, images, half=0.5, leaf=0.01):
    """The merged, thinned cloud of one pose set.  images: [m,H,W,3] BGR or a callable k -> [H,W,3]."""
    scan_times = np.asarray(scan_times, np.float64)
    poses = np.asarray(scan_poses, np.float64).reshape(-1, 12)
    world = [world_points(c, T) for c, T in zip(clouds, poses)]
    xs, cs = [], []
    for k, tk in enumerate(np.asarray(image_times, np.float64)):
        use = [i for i in range(len(world)) if not abs(scan_times[i] - tk) > half]
        pw = np.concatenate([world[i] for i in use]) if use else np.zeros((0, 3), np.float32)
        if len(pw) == 0:
            continue
        img = images(k) if callable(images) else images[k]
        x, c = colorize_image(pw, np.asarray(Rcw)[k], np.asarray(tcw)[k], intr, W, H, img)
        xs.append(x); cs.append(c)
    xyz = np.concatenate(xs) if xs else np.zeros((0, 3), np.float32)
    rgb = np.concatenate(cs) if cs else np.zeros((0, 3), np.uint8)
    return down_sampling_voxel2(xyz, rgb, leaf)


def pattern_image(W, H):
    """The stand-in imread of oracle/shim: (b, g, r) = (x, y, x + y) mod 256."""
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    return np.stack([x % 256, y % 256, (x + y) % 256], -1).astype(np.uint8)


def points3d_lines(xyz, rgb):
    """points3D.txt rows without the leading index (:2128-2136): "x y z r g b 0" with 6 decimals."""
    return [f"{x:.6f} {y:.6f} {z:.6f} {int(r)} {int(g)} {int(b)} 0" for (x, y, z), (r, g, b) in
            zip(np.asarray(xyz, np.float32).astype(np.float64), np.asarray(rgb, np.uint8))]
