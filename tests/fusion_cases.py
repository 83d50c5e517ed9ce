"""Inputs of the depth rendering (csrc/fusion.hip: lvba_depth_render) and of the per-track fusion (csrc/fusion_device.h:
fuse_track) at the edges of their rules, with the expectations that follow from each rule by hand.  Shared by
tests/test_fusion_cases_host.py (the cases against the oracle and the host build of the device header, and the conditions
the cases are built to meet) and tests/test_gpu_fusion_edges.py (the kernels).  TEST INFRASTRUCTURE ONLY: numpy, no GPU, no
product import; the only oracle call is fusion_oracle.render_depth, which draws the wall the track cases look at.

DEPTH CASES.  dict(name, clouds, scan_poses [n,12], scan_times, image_times, Rcw, tcw, intr, W, H, half_window, voxel,
drawn, empty, count).  drawn: [(image, row, col, float32 depth or None)] pixels the rule fills (with that value where it is
known); empty: [(image, row, col)] pixels the rule leaves 0; count: per image the number of filled pixels, or None where no
hand count exists.  Unless a case says otherwise the camera is intr = (64, 64, 32, 24, 0, 0, 0, 0), 64 x 48, Rcw = I, tcw = 0,
the scan poses are identities or translations, so u = 64 X / Z + 32, v = 64 Y / Z + 24.
    D1 pixel_truncation    (int)u truncates towards zero: u in (-1, 0) lands in column 0, u = -1 and u = W are outside
    D2 near_plane          Z >= 1e-3 is drawn (float32(1e-3) is above the double 1e-3), the float below it, 0 and Z < 0 are not
    D3 voxel_key_*         the reference's key (float quotient, -1 if negative, truncation) puts x = -0.5 into voxel -2, not -1
    D4 one_pixel_contention 4096 points of 4 scans on one pixel, the smallest depth 16 times
    D5 windows_*           inclusive window bounds, two scans of one time, an empty scan, windows that hold nothing
    D6 sizes_*             images of 4, 256, 255 and 258 pixels, 1 / 255 / 256 / 257 map points
    D7 distorted_off_axis  the general path: distortion, a rotated camera, points behind it and far off axis

TRACK CASES.  dict(name, off, img, uv, depth [40,H,W] float32 (to be uploaded), Rcw, tcw, intr, ...).  Forty cameras stand on
an arc of +-35 degrees, 7 m from the middle of a gently corrugated wall (6.75 .. 7.25 m) and look at that middle; image id
m stands at arc position 17 m mod 40, so that ids which are neighbours modulo a small prime are not neighbours on the arc.
The depth images are the oracle's rendering of a dense sampling of the wall (T6, T7 and T9 then overwrite single pixels).
    T1 block_edges         129 tracks of every kind the options tell apart; prefixes of 1, 63, 64, 65 (fuse_kernel: 64 per block)
    T2 short_and_empty     tracks of 0, 1, 2 observations before, between and after good ones
    T3 image_counts        3 observations in 3 images, 3 in 2, 4 in 3, 4 in 4, and 5 images of which the view filter keeps 3
    T4 bucket_collisions   image ids congruent modulo the bucket count of their reserve(), observation order shuffled
    T5 long_track          120 observations (3 per image) between two 3-observation tracks
    T6 pixel_edges         one observation at u = v = 0, -0.0, W - 1, just below W - 1, NaN, +-inf, next to a zero-depth pixel
    T7 anchor              the first valid observation is the anchor even when it is the wrong one; 0.10 m and 0.14 m from it
    T8 options             T1 under other obser_thr / min_view_angle_deg / reproj_mean_thr_px
    T9 selection           both candidates pass; either may have the smaller mean
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import fusion_oracle as fo

f32 = np.float32
I12 = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
PIN_INTR = np.array([64.0, 64.0, 32.0, 24.0, 0.0, 0.0, 0.0, 0.0])
PIN_W, PIN_H = 64, 48
# the distorted camera and the body -> camera rotation of tests/test_gpu_fusion.py
RCB = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
INTR = np.array([120.0, 118.0, 80.0, 60.0, 0.02, -0.005, 0.001, -0.0005])
W, H = 160, 120


def _trans(t):
    return np.concatenate([np.eye(3).reshape(-1), np.asarray(t, np.float64)])


def _depth_case(name, clouds, scan_times, image_times, drawn=(), empty=(), count=None, scan_poses=None, Rcw=None, tcw=None,
                intr=PIN_INTR, width=PIN_W, height=PIN_H, half_window=0.5, voxel=0.5):
    n_img = len(image_times)
    clouds = [np.asarray(c, f32).reshape(-1, 3) for c in clouds]
    assert sum(len(c) for c in clouds) < 10000
    return dict(name=name, clouds=clouds,
                scan_poses=np.array([I12] * len(clouds)) if scan_poses is None else np.asarray(scan_poses, np.float64),
                scan_times=np.asarray(scan_times, np.float64), image_times=np.asarray(image_times, np.float64),
                Rcw=np.array([np.eye(3)] * n_img) if Rcw is None else np.asarray(Rcw, np.float64),
                tcw=np.zeros((n_img, 3)) if tcw is None else np.asarray(tcw, np.float64),
                intr=np.asarray(intr, np.float64), W=width, H=height, half_window=half_window, voxel=voxel,
                drawn=list(drawn), empty=list(empty), count=count)


def _pin_point(u, v, z=1.0):
    """The float32 point that the pinhole camera sees at (u, v) with depth z."""
    return [f32((u - 32.0) / 64.0 * z), f32((v - 24.0) / 64.0 * z), f32(z)]


def pixel_truncation():
    one = f32(1.0)
    inside = [((-0.5, 10.5), (10, 0)), ((63.5, 12.5), (12, 63)), ((5.5, -0.5), (0, 5)), ((7.5, 47.5), (47, 7)),
              ((0.0, 0.0), (0, 0)), ((63.999, 47.999), (47, 63))]
    # where a clamping or rounding rule would put them: (11, 0), (13, 63), (0, 6), (47, 8)
    outside = [((-1.0, 11.5), (11, 0)), ((64.0, 13.5), (13, 63)), ((6.5, -1.0), (0, 6)), ((8.5, 48.0), (47, 8))]
    pts = [_pin_point(*uv) for uv, _ in inside + outside]
    return _depth_case("pixel_truncation", [pts], [0.0], [0.0], drawn=[(0, r, c, one) for _, (r, c) in inside],
                       empty=[(0, r, c) for _, (r, c) in outside], count=[len(inside)])


def near_plane():
    z0 = f32(1e-3)
    below = np.nextafter(z0, f32(0.0))
    assert float(z0) >= 1e-3 > float(below)
    k = 8.5 / 64.0                                                          # u = 40.5 for Z > 0, 23.5 for Z < 0
    pts = [[f32(k * float(z0)), f32(0.0), z0],                              # row 24: drawn
           [f32(k * float(below)), f32(float(below) * 4.5 / 64.0), below],  # row 28: not drawn
           [f32(0.01), f32(0.02), f32(0.0)], [f32(k), f32(8.5 / 64.0), f32(-1.0)],
           _pin_point(10.5, 10.5, 2.0)]
    return _depth_case("near_plane", [pts], [0.0], [0.0], drawn=[(0, 24, 40, z0), (0, 10, 10, f32(2.0))],
                       empty=[(0, 28, 40), (0, 32, 40), (0, 32, 23), (0, 15, 23), (0, 15, 40)], count=[2])


def voxel_key_at_negative_multiples(axis):
    """Scan A (in the window) touches voxel -2 of `axis` with a point at exactly -0.5; scan B (out of the window) has a point
    at -0.75 (voxel -2: drawn with A's voxel) and one at -0.3 (voxel -1: not drawn -- a floor(x / 0.5) key would put -0.5
    into voxel -1 and draw it)."""
    other = (0.125, 0.25)                                                    # voxel 0 of both other axes

    def point(a):
        p = list(other)
        p.insert(axis, a)
        return np.array(p, f32)
    A, B1, B2 = point(-0.5), point(-0.75), point(-0.3)
    tc = np.array([0.0, 0.0, 2.0])

    def pixel(p):
        q = p.astype(np.float64) + tc
        u, v = 64.0 * q[0] / q[2] + 32.0, 64.0 * q[1] / q[2] + 24.0
        assert 0.05 < u % 1 < 0.95 and 0.05 < v % 1 < 0.95                  # nowhere near a pixel border
        return int(v), int(u), f32(q[2])
    pa, pb1, pb2 = pixel(A), pixel(B1), pixel(B2)
    assert len({pa[:2], pb1[:2], pb2[:2]}) == 3
    c = _depth_case("voxel_key_axis%d" % axis, [[A], [B1, B2]], [0.0, 100.0], [0.0], tcw=[tc],
                    drawn=[(0,) + pa, (0,) + pb1], empty=[(0,) + pb2[:2]], count=[2])
    c["key_points"], c["axis"] = np.array([A, B1, B2], np.float64), axis
    return c


def one_pixel_contention():
    rng = np.random.default_rng(404)
    z = np.concatenate([np.full(16, 1.0), 1.0 + np.arange(1, 4081) / 1024.0])      # exact floats, 4081 distinct values
    assert len(z) == 4096 and len(np.unique(z.astype(f32))) == 4081
    z = rng.permutation(z)
    a = 0.5 / 64.0                                                           # u = 32.5, v = 24.5 for every one of them
    world = np.stack([(z * a).astype(f32).astype(np.float64), (z * a).astype(f32).astype(np.float64), z], 1)
    assert len({tuple(k) for k in fo.voxel_keys(world, 0.5)}) >= 8
    tz = [0.0, 1.0, -1.0, 2.0]                                               # scan s stands at (0, 0, tz[s]): z - tz is exact
    clouds = [world[s::4] - np.array([0.0, 0.0, tz[s]]) for s in range(4)]
    clouds[1] = np.concatenate([clouds[1], [np.array(_pin_point(10.5, 10.5, 3.0), np.float64) - [0, 0, 1.0]]])
    clouds[2] = np.concatenate([clouds[2], [np.array(_pin_point(10.5, 10.5, 2.0), np.float64) - [0, 0, -1.0]]])
    return _depth_case("one_pixel_contention", clouds, [0.0, 0.1, 0.2, 0.3], [0.1],
                       scan_poses=[_trans([0, 0, t]) for t in tz], drawn=[(0, 24, 32, f32(1.0)), (0, 10, 10, f32(2.0))], count=[2])


def windows():
    """Two cases (half_window_s is an argument of the call).  Scan s fills four pixels of its own from a voxel of its own."""
    times = [0.0, 1.0, 1.0, 2.0, 4.0, 4.5]
    clouds, pix = [], []
    for s in range(6):
        x0 = -1.5 + 0.5 * s
        pts = [[f32(x0 + dx), f32(dy), f32(4.1)] for dx in (0.15, 0.35) for dy in (0.15, 0.35)]
        px = []
        for p in pts:
            u, v = 64.0 * float(p[0]) / float(p[2]) + 32.0, 64.0 * float(p[1]) / float(p[2]) + 24.0
            assert 0.02 < u % 1 < 0.98 and 0.02 < v % 1 < 0.98
            px.append((int(v), int(u)))
        assert len(set(px)) == 4
        clouds.append(pts if s != 3 else np.zeros((0, 3), f32))
        pix.append(px)
    assert len({p for px in pix for p in px}) == 24
    assert len({tuple(fo.voxel_keys(np.array(c, np.float64), 0.5)[0]) for c in clouds if len(c)}) == 5
    out = []
    for half, imgs in ((0.5, [(-1.0, ()), (0.5, (0, 1, 2)), (3.0, ()), (100.0, ())]), (0.25, [(2.0, ()), (4.25, (4, 5))])):
        drawn, empty, count = [], [], []
        for m, (_, scans) in enumerate(imgs):
            for s in range(6):
                if s == 3:
                    continue
                if s in scans:
                    drawn += [(m, r, c, f32(4.1)) for r, c in pix[s]]
                else:
                    empty += [(m, r, c) for r, c in pix[s]]
            count.append(4 * len(scans))
        out.append(_depth_case("windows_half%g" % half, clouds, times, [t for t, _ in imgs], drawn=drawn, empty=empty,
                               count=count, half_window=half))
    return out


def sizes():
    """Every image size with every point count: the render's work items (= points: every voxel is in the window) and the
    finishing pass over n_images * W * H pixels straddle the 256-thread block."""
    out = []
    for (w, h, n_img) in ((2, 2, 1), (16, 16, 1), (17, 5, 3), (43, 6, 1)):
        for P in (1, 255, 256, 257):
            rng = np.random.default_rng(1000 * w + P)
            z = rng.uniform(1.0, 2.0, P)
            pts = np.stack([rng.uniform(-0.4, 0.4, P) * z, rng.uniform(-0.4, 0.4, P) * z, z], 1).astype(f32)
            cut = P // 3
            tcw = np.array([[0.03 * m, -0.02 * m, 0.0] for m in range(n_img)])
            out.append(_depth_case("sizes_%dx%dx%d_P%d" % (w, h, n_img, P), [pts[:cut], pts[cut:]], [0.0, 0.2], [0.1] * n_img,
                                   tcw=tcw, intr=[w, h, w / 2.0, h / 2.0, 0, 0, 0, 0], width=w, height=h))
    return out


def distorted_off_axis():
    """No hand list: 2 000 points in a +-20 m cube around a rotated, distorted camera.  The third scan is out of the window
    and repeats points of the first with a jitter of up to 0.3 m, so about half of its points fall into a drawn voxel."""
    rng = np.random.default_rng(77)
    Cw = np.array([1.5, -2.25, 0.75])
    yaw = 0.3
    Rwb = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    R = RCB @ Rwb.T
    world = Cw + rng.uniform(-20.0, 20.0, (1400, 3))
    tB = np.array([0.5, -1.0, 0.25])
    cA, cB = world[:800].astype(f32), (world[800:] - tB).astype(f32)
    cC = (cA[:600].astype(np.float64) + rng.uniform(-0.3, 0.3, (600, 3))).astype(f32)
    return _depth_case("distorted_off_axis", [cA, cB, cC], [0.0, 0.25, 100.0], [0.1, 100.2], Rcw=[R, R], tcw=[-R @ Cw, -R @ Cw],
                       scan_poses=[I12, _trans(tB), I12], intr=INTR, width=W, height=H)


@functools.lru_cache(maxsize=None)
def depth_cases():
    out = [pixel_truncation(), near_plane()] + [voxel_key_at_negative_multiples(a) for a in range(3)]
    out += [one_pixel_contention()] + windows() + sizes() + [distorted_off_axis()]
    return tuple(out)


def oracle_depth(c):
    return fo.render_depth(c["clouds"], c["scan_poses"], c["scan_times"], c["image_times"], c["Rcw"], c["tcw"], c["intr"],
                           c["W"], c["H"], half_w=c["half_window"], vox=c["voxel"])


def check_depth_lists(c, img):
    """img [n_images, H, W] against the case's hand lists."""
    for m, r, col, val in c["drawn"]:
        assert img[m, r, col] > 0, (c["name"], "not drawn", m, r, col)
        if val is not None:
            assert img[m, r, col] == val, (c["name"], m, r, col, img[m, r, col], val)
    for m, r, col in c["empty"]:
        assert img[m, r, col] == 0, (c["name"], "drawn", m, r, col, img[m, r, col])
    if c["count"] is not None:
        assert [int((img[m] > 0).sum()) for m in range(len(img))] == list(c["count"]), c["name"]


# ------------------------------------------------------------------------------------------------------------ track cases
N_CAMS = 40
ARC_STEP_DEG = 1.8


def arc_position(m):
    return (17 * m) % N_CAMS


def wall_x(y, z):
    return 7.0 + 0.25 * np.sin(0.9 * y) * np.cos(0.7 * z)


@functools.lru_cache(maxsize=None)
def rig():
    """Rcw [40,3,3], tcw [40,3] of the arc."""
    Rcw, tcw = [], []
    for m in range(N_CAMS):
        th = np.radians((arc_position(m) - (N_CAMS - 1) / 2.0) * ARC_STEP_DEG)
        Rwb = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        C = np.array([7.0, 0.0, 0.0]) - 7.0 * np.array([np.cos(th), np.sin(th), 0.0]) + np.array([0.0, 0.0, 0.1 * (m % 3)])
        R = RCB @ Rwb.T
        Rcw.append(R); tcw.append(-R @ C)
    Rcw, tcw = np.array(Rcw), np.array(tcw)
    Rcw.setflags(write=False); tcw.setflags(write=False)
    return Rcw, tcw


@functools.lru_cache(maxsize=None)
def wall_depth():
    """The oracle's depth images of the wall sampled every 3 cm (read-only; shared by every track case)."""
    Rcw, tcw = rig()
    y, z = np.meshgrid(np.arange(-7.0, 7.0, 0.03), np.arange(-4.5, 4.5, 0.03), indexing="ij")
    cloud = np.stack([wall_x(y, z), y, z], -1).reshape(-1, 3).astype(f32)
    d = fo.render_depth([cloud], [I12], [0.0], [0.0] * N_CAMS, Rcw, tcw, INTR, W, H, half_w=1.0)
    d.setflags(write=False)
    return d


def project(m, X):
    """Pixel (double) of the world point X in image m: the camera model of include/utils.hpp, restated."""
    Rcw, tcw = rig()
    fx, fy, cx, cy, k1, k2, p1, p2 = INTR
    q = Rcw[m] @ X + tcw[m]
    x, y = q[0] / q[2], q[1] / q[2]
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
    yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
    return np.array([fx * xd + cx, fy * yd + cy]), q[2]


def landmark(rng):
    y, z = rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0)
    return np.array([wall_x(y, z), y, z])


def observe(X, images, rng, noise):
    """[(image, uv float32)] of X in `images` (repeats allowed) with Gaussian pixel noise."""
    out = []
    for m in images:
        p, _ = project(int(m), X)
        assert 3 < p[0] < W - 4 and 3 < p[1] < H - 4
        out.append((int(m), (p + noise * rng.standard_normal(2)).astype(f32)))
    return out


def spread_images(rng, n, lo=0, hi=N_CAMS):
    """n image ids at distinct arc positions drawn from [lo, hi)."""
    pos = rng.choice(np.arange(lo, hi), n, replace=False)
    inv = {arc_position(m): m for m in range(N_CAMS)}
    return [inv[int(p)] for p in pos]


def images_at(positions):
    inv = {arc_position(m): m for m in range(N_CAMS)}
    return [inv[int(p)] for p in positions]


def pack(tracks):
    off, img, uv = [0], [], []
    for t in tracks:
        for m, p in t:
            img.append(m); uv.append(p)
        off.append(len(img))
    return np.array(off, np.int64), np.array(img, np.int32), np.array(uv, f32).reshape(-1, 2)


def _track_case(name, tracks, depth=None, **extra):
    Rcw, tcw = rig()
    off, img, uv = pack(tracks)
    assert len(tracks) <= 200
    c = dict(name=name, off=off, img=img, uv=uv, depth=wall_depth() if depth is None else depth, Rcw=Rcw, tcw=tcw, intr=INTR)
    c.update(extra)
    return c


def poke(depth, m, uv, d):
    """The four pixels the bilinear fetch at uv reads, set to d: the fetch then returns d (to float rounding)."""
    x, y = int(np.floor(uv[0])), int(np.floor(uv[1]))
    depth[m, y:y + 2, x:x + 2] = f32(d)
    return (m, y, x)


def good_track(rng, n_images, noise=0.25, lo=0, hi=N_CAMS):
    X = landmark(rng)
    return observe(X, spread_images(rng, n_images, lo, hi), rng, noise)


@functools.lru_cache(maxsize=None)
def block_edges():
    """129 tracks, none empty, of the kinds the options of T8 tell apart (kind = t mod 8):
       0, 1  6..12 images anywhere on the arc, 0.25 px noise      5  6 images within 5 arc positions (< 8 degrees)
       2     2 images                                             6  8 images, 1 px noise
       3     3 images                                             7  8 images, 6 px noise
       4     4 images"""
    rng = np.random.default_rng(2024)
    tracks = []
    for t in range(129):
        k = t % 8
        if k in (0, 1):
            tr = good_track(rng, int(rng.integers(6, 13)))
        elif k in (2, 3, 4):
            tr = good_track(rng, k)
        elif k == 5:
            lo = int(rng.integers(0, N_CAMS - 5))
            tr = observe(landmark(rng), images_at(rng.permutation(np.arange(lo, lo + 5))), rng, 0.25)
        else:
            tr = good_track(rng, 8, noise=1.0 if k == 6 else 6.0)
        tracks.append(tr)
    return _track_case("block_edges", tracks, prefixes=(1, 63, 64, 65))


def short_and_empty():
    rng = np.random.default_rng(31)
    g = lambda: good_track(rng, int(rng.integers(5, 9)))
    tracks = [[], g(), good_track(rng, 1), g(), good_track(rng, 2), [], [], g(), good_track(rng, 2), g(), good_track(rng, 1), []]
    good = [1, 3, 7, 9]
    return _track_case("short_and_empty", tracks, good=good, dropped=[t for t in range(len(tracks)) if t not in good])


# arc positions of the 5-image track of T3 whose view filters keep exactly three (found by search; asserted from the trace)
KEEPS_THREE_POSITIONS = (12, 14, 16, 19, 20)


def image_counts(keeps_three=KEEPS_THREE_POSITIONS, seed=5):
    """expect: track -> (status with depth, status with depth=None)."""
    rng = np.random.default_rng(seed)
    wide = images_at([2, 13, 24, 35])                                        # about 20 degrees apart
    X = [landmark(rng) for _ in range(6)]
    tracks = [observe(X[0], wide[:3], rng, 0.2),                             # 0: 3 in 3
              observe(X[1], [wide[0], wide[1], wide[0]], rng, 0.2),          # 1: 3 in 2
              observe(X[2], [wide[0], wide[1], wide[0], wide[2]], rng, 0.2),   # 2: 4 in 3, far apart
              observe(X[3], images_at([20, 21, 20, 22]), rng, 0.2),          # 3: 4 in 3, within 3.6 degrees
              observe(X[4], wide, rng, 0.2),                                 # 4: 4 in 4
              observe(X[5], images_at(keeps_three), rng, 0.2)]               # 5: 5 images, the view filters keep 3
    # 4 observations in 3 images can never be triangulated (4 images needed); far apart the depth candidate takes the
    # track as it takes 3 in 3, within 3.6 degrees the view filter leaves one observation and nothing takes it
    expect = {0: (2, 0), 1: (0, 0), 2: (2, 0), 3: (0, 0), 4: (None, 1), 5: (2, 0)}
    return _track_case("image_counts", tracks, expect=expect, keeps_three=5)


def bucket_collisions():
    """Every track: n observations (5..12), so reserve(n) gives B = 5, 7, 11 or 13 buckets; its images are a run of ids that are
    congruent modulo B (they share one bucket, which is walked latest first) and a few others; duplicates fill up to n."""
    rng = np.random.default_rng(1213)
    tracks = []
    for t in range(150):
        n = int(rng.integers(5, 13))
        B = fo.umap_bucket_count(n)
        r = int(rng.integers(0, B))
        same = [m for m in range(r, N_CAMS, B)]
        rng.shuffle(same)
        n_same = min(len(same), int(rng.integers(2, 5)))
        n_img = int(rng.integers(max(4, n_same + 1), n + 1))
        others = [m for m in rng.permutation(N_CAMS) if m % B != r][:max(0, n_img - n_same)]
        images = same[:n_same] + [int(m) for m in others]
        images = images + [images[int(i)] for i in rng.integers(0, len(images), n - len(images))]
        rng.shuffle(images)
        assert len(images) == n
        tracks.append(observe(landmark(rng), images, rng, 0.25))
    return _track_case("bucket_collisions", tracks)


def long_track():
    rng = np.random.default_rng(120)
    images = [m for m in range(N_CAMS) for _ in range(3)]
    rng.shuffle(images)
    wide = images_at([3, 15, 27])
    tracks = [observe(landmark(rng), wide, rng, 0.2), observe(landmark(rng), images, rng, 0.3),
              observe(landmark(rng), images_at([6, 20, 33]), rng, 0.2)]
    return _track_case("long_track", tracks, neighbours=[0, 2], long=1)


PIXEL_EDGE_KINDS = ("zero", "minus_zero", "w_minus_1", "below_w_minus_1", "nan", "plus_inf", "minus_inf", "zero_neighbour")
# kinds whose pixel is inside the fetch's range (a depth point exists, far from the landmark)
PIXEL_EDGE_IN_RANGE = ("zero", "minus_zero", "below_w_minus_1")


def pixel_edges():
    """Two tracks per kind, six images each; the special observation is the 4th of the first track and the 1st of the second.
    Its image is the one in the middle of the arc, whose corner pixels see the wall.  In range it gets a depth point metres
    from the landmark: as the 4th observation that point fails the 0.12 m test and the track succeeds on the others; as the 1st
    it IS the anchor, every other point fails, and the depth candidate is lost (not_depth_fused).  Out of range, non-finite or
    next to a zero depth it has no depth point and the track succeeds either way (must_succeed); a pixel that is not a true
    observation is in no winner's kept list (special_unkept: (track, observation))."""
    rng = np.random.default_rng(66)
    depth = wall_depth().copy()
    mid = images_at([20])[0]
    assert (depth[mid, :2, :2] > 0).all() and (depth[mid, :2, W - 2:] > 0).all()
    tracks, special, must_succeed, not_depth_fused, special_unkept = [], [], [], [], []
    for kind in PIXEL_EDGE_KINDS:
        for where in (3, 0):
            others = [m for m in spread_images(rng, 8) if m != mid][:5]
            tr = observe(landmark(rng), others, rng, 0.2)
            p, _ = project(mid, landmark(rng))
            uv = {"zero": (0.0, 0.0), "minus_zero": (-0.0, -0.0), "w_minus_1": (W - 1.0, 0.0),
                  "below_w_minus_1": (np.nextafter(f32(W - 1), f32(0)), 0.0), "nan": (np.nan, p[1]), "plus_inf": (np.inf, p[1]),
                  "minus_inf": (p[0], -np.inf), "zero_neighbour": None}[kind]
            if uv is None:
                uv = observe(landmark(rng), [mid], rng, 0.2)[0][1]
                x, y = int(np.floor(uv[0])), int(np.floor(uv[1]))
                depth[mid, y + 1, x + 1] = 0.0
            tr.insert(where, (mid, np.array(uv, f32)))
            special.append((len(tracks), where))
            if where == 0 and kind in PIXEL_EDGE_IN_RANGE:
                not_depth_fused.append(len(tracks))
            else:
                must_succeed.append(len(tracks))
                if kind != "zero_neighbour":                                 # that one is a true observation: it may be kept
                    special_unkept.append((len(tracks), where))
            tracks.append(tr)
    assert np.signbit(tracks[2][3][1]).all()
    return _track_case("pixel_edges", tracks, depth=depth, special=special, must_succeed=must_succeed,
                       not_depth_fused=not_depth_fused, special_unkept=special_unkept)


def anchor():
    """Depth images with hand-set pixels: every observation's four fetch pixels hold the landmark's true depth in that
    image, plus `delta`.  Tracks 0..5 (6 images, 0.1 px noise): the first observation is 1 m off, so it is the anchor, no other
    point is within 0.12 m, the depth candidate is lost and the triangulation decides.  Tracks 6..11: three images far apart, which
    cannot be triangulated, so the depth candidate alone decides; the last observation is 0.10 m off in tracks 6..8 (an inlier:
    fused, X pulled a third of 0.10 m along its ray) and 0.14 m off in tracks 9..11 (no inlier: two images left, dropped).  (A
    track cannot show both: a second observation of one image reads the same four depth pixels as the first.)"""
    rng = np.random.default_rng(7007)
    depth = wall_depth().copy()
    tracks, used = [], set()
    for t in range(12):
        while True:
            X = landmark(rng)
            if t < 6:
                images = spread_images(rng, 6)
            else:
                A, B, C = images_at([int(rng.integers(0, 8)), int(rng.integers(16, 24)), int(rng.integers(32, 40))])
                images = [A, B, C]
            obs = observe(X, images, rng, 0.1)
            cells = {(m, int(np.floor(p[1])) + dy, int(np.floor(p[0])) + dx) for m, p in obs for dy in (0, 1) for dx in (0, 1)}
            if not (cells & used):
                break
        used |= cells
        delta = [1.0, 0, 0, 0, 0, 0] if t < 6 else [0, 0, 0.10 if t < 9 else 0.14]
        for (m, p), dl in zip(obs, delta):
            poke(depth, m, p, project(m, X)[1] + dl)
        tracks.append(obs)
    return _track_case("anchor", tracks, depth=depth, wrong_anchor=list(range(6)), near=[6, 7, 8], far=[9, 10, 11])


OPTION_SETS = (dict(obser_thr=2), dict(obser_thr=4), dict(obser_thr=5), dict(min_view_angle_deg=0.5), dict(min_view_angle_deg=30.0),
               dict(reproj_mean_thr_px=0.5), dict(reproj_mean_thr_px=1e9))


def options():
    c = dict(block_edges())
    c.update(name="options", option_sets=OPTION_SETS)
    return c


def selection():
    """Both candidates pass on most of these tracks.  Even tracks: 8 images, one observation each, 0.3..1.2 px noise and the
    wall's own depth: the DLT fits the pixels and usually has the smaller mean.  Odd tracks: three of the 8 images have a first
    observation that is 2..4 px off AND 0.5 m off in depth, followed by a good one: the triangulation takes the first
    observation of every image, the depth candidate the first INLIER, so its mean is usually the smaller one."""
    rng = np.random.default_rng(909)
    depth = wall_depth().copy()
    tracks = []
    for t in range(80):
        X = landmark(rng)
        images = spread_images(rng, 8)
        obs = observe(X, images, rng, rng.uniform(0.3, 1.2))
        if t % 2:
            for i in (2, 4, 6):
                m = obs[i][0]
                p, zc = project(m, X)
                bad = (p + rng.uniform(2.0, 4.0) * np.array([np.cos(t + i), np.sin(t + i)])).astype(f32)
                poke(depth, m, bad, zc + 0.5)
                obs.insert(i, (m, bad))
        tracks.append(obs)
    return _track_case("selection", tracks, depth=depth)


@functools.lru_cache(maxsize=None)
def track_cases():
    return (block_edges(), short_and_empty(), image_counts(), bucket_collisions(), long_track(), pixel_edges(), anchor(),
            selection())


def sub_tracks(c, which):
    """(off, img, uv) of the tracks `which` of a case alone."""
    off, img, uv = c["off"], c["img"], c["uv"]
    sel = np.concatenate([np.arange(off[t], off[t + 1]) for t in which] + [np.zeros(0, np.int64)]).astype(np.int64)
    noff = np.concatenate([[0], np.cumsum([off[t + 1] - off[t] for t in which])]).astype(np.int64)
    return noff, img[sel], uv[sel]


# ------------------------------------------------------------------------------------------- the oracle's answers, computed once
_ORACLE = {}


def case_by_name(name):
    return {c["name"]: c for c in track_cases() + (options(),)}[name]


def oracle_tracks(c, with_depth, **opts):
    """(status, X, mean, kept, traces) of the oracle for a track case; opts in the API's names.  Cached, read-only."""
    key = (c["name"], bool(with_depth), tuple(sorted(opts.items())))
    if key not in _ORACLE:
        kw = dict(opts)
        if "reproj_mean_thr_px" in kw:
            kw["reproj_thr"] = kw.pop("reproj_mean_thr_px")
        n = len(c["off"]) - 1
        st, X, err, kept, traces = np.zeros(n, np.uint8), np.zeros((n, 3)), np.full(n, np.inf), np.zeros(len(c["img"]), np.uint8), []
        for t in range(n):
            a, b = int(c["off"][t]), int(c["off"][t + 1])
            tr = {}
            st[t], X[t], err[t], kept[a:b] = fo.fuse_track(c["img"][a:b], c["uv"][a:b], c["depth"] if with_depth else None, c["Rcw"],
                                                           c["tcw"], c["intr"], trace=tr, **kw)
            traces.append(tr)
        for v in (st, X, err, kept):
            v.setflags(write=False)
        _ORACLE[key] = (st, X, err, kept, tuple(traces))
    return _ORACLE[key]


def assert_tracks_match(got, want, what=""):
    """The project's bars (tests/test_gpu_fusion.py): status and kept exact, X and mean to 1e-9, dropped rows zeros and +inf."""
    np.testing.assert_array_equal(got[0], want[0], err_msg=str(what))
    np.testing.assert_array_equal(got[3], want[3], err_msg=str(what))
    ok = want[0] > 0
    if ok.any():
        assert np.abs(got[1][ok] - want[1][ok]).max() <= 1e-9, what
        assert np.abs(got[2][ok] - want[2][ok]).max() <= 1e-9, what
    assert np.isinf(got[2][~ok]).all() and (got[2][~ok] > 0).all() and not got[1][~ok].any(), what


def check_track_lists(c, got, with_depth):
    """(status, X, mean, kept) of any implementation against the case's hand-derived outcomes."""
    st, kept, off = got[0], got[3], c["off"]
    name = c["name"]
    if name == "short_and_empty":
        assert (st[c["dropped"]] == 0).all() and (st[c["good"]] > 0).all()
    elif name == "image_counts":
        for t, e in c["expect"].items():
            want = e[0 if with_depth else 1]
            assert want is None or st[t] == want, (name, t, st[t], want)
    elif name == "long_track":
        assert st[c["long"]] > 0 and (st[c["neighbours"]] == (2 if with_depth else 0)).all()
    elif name == "pixel_edges" and with_depth:
        assert (st[c["must_succeed"]] > 0).all() and (st[c["not_depth_fused"]] != 2).all()
        assert not any(kept[off[t] + o] for t, o in c["special_unkept"])
    elif name == "anchor":
        assert (st[c["wrong_anchor"]] == 1).all()
        if with_depth:
            assert (st[c["near"]] == 2).all() and (st[c["far"]] == 0).all()
            assert all(kept[off[t]:off[t + 1]].all() for t in c["near"])
