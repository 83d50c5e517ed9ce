"""Fixture of the colour-fusion tests (tests/test_photo_host.py on the CPU, tests/test_gpu_photo.py on the GPU): the room of
covis_cases.room(size), both sizes, all 21 images (the twin, the image with 70 % holes and the empty one included).  The points
are the planted points rounded to float; the images are rendered here: every pixel's ray is cast with covis_cases.cast to its
wall point, which takes a smooth planted colour of its world position, rounded to a byte.  Seeded; nothing is committed.

Margin condition (as in covis_cases.py): a condition on the fixture, checked on the CPU, not a tolerance on the device.
`check_margins` asserts, for every size and option set the tests use, that every evaluated in-image comparison, every Z against
its occlusion bound and every Z against max_depth is at least match_cases.MIN_MARGIN (relative) away from its bound, and that
every sampled u, v is at least TEXEL_MARGIN px from the nearest multiple of 1/256: the projection's doubles differ between numpy
and the device by a few ulps, about 1e-12 px at these image sizes, and the margin is 100 times that."""
import functools

import numpy as np

import covis_cases as cc
import covis_oracle as co
import match_cases as mc
import photo_oracle as po

TEXEL_MARGIN = 1e-10
TEXTURE_FREQ = 0.8                                                    # rad / m: about one and a half periods across the room
# the option sets the GPU tests run; `depth` is the fixture's switch (False: no depth set), the rest are lvba_photo_opts
OPTION_SETS = (dict(), dict(depth=False), dict(holes=1), dict(max_depth=5.0), dict(min_views=3),
               dict(occlusion_rel=0.0, occlusion_abs=0.02))
POINT_COUNTS = (0, 1, 63, 64, 255, 256, 257, cc.N_PLANTED)            # chunk edges of the 256-point workgroup
M_VALUES = cc.M_VALUES


def planted_colour(P):
    """float64 [n, 3] (b, g, r) in [27.5, 227.5]: a smooth function of the world position"""
    f = TEXTURE_FREQ
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return 127.5 + 100.0 * np.stack([np.sin(f * (x + 0.5 * y) + 0.3), np.cos(f * (z + 0.3 * x) - 0.2), np.sin(f * (1.5 * y + 0.7 * z) + 1.0)], 1)


def render_image(intr, Rcw, C, W, H):
    """uint8 [H, W, 3]: the planted colour of the wall point along the undistorted ray of every pixel"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y, ok = co.undistort(intr, u.ravel(), v.ravel())
    assert ok.all()
    dirs = np.stack([x, y, np.ones_like(x)], 1) @ Rcw
    s = cc.cast(C, dirs)
    assert np.isfinite(s).all()                                       # the room is closed
    return np.floor(planted_colour(C + s[:, None] * dirs) + 0.5).astype(np.uint8).reshape(H, W, 3)


def centres(Rcw, tcw):
    return -np.einsum("nji,nj->ni", Rcw, tcw)


@functools.lru_cache(None)
def scene(size=0):
    """covis_cases.room(size) with points float32 [4200, 3], colour float64 [4200, 3] (b, g, r) and images uint8 [21, H, W, 3]"""
    r = dict(cc.room(size))
    C = centres(r["Rcw"], r["tcw"])
    r["points"] = np.ascontiguousarray(r["planted"].astype(np.float32))
    r["colour"] = planted_colour(r["points"].astype(np.float64))
    r["images"] = np.ascontiguousarray(np.stack([render_image(r["intr"], r["Rcw"][k], C[k], r["W"], r["H"]) for k in range(cc.N_IMAGES)]))
    r["C"] = C
    return r


def split(kw):
    """an option set -> (use the depth set, the library's options)"""
    kw = dict(kw)
    return kw.pop("depth", True), kw


def key_of(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(None)
def _expected(size, key):
    s = scene(size)
    with_depth, opts = split(dict(key))
    return po.evaluate(s["points"], s["images"], s["depth"] if with_depth else None, s["intr"], s["Rcw"], s["tcw"], **opts)


def expected(size, **kw):
    """the oracle on all points and all 21 images under an option set (computed once; do not write into it)"""
    return _expected(size, key_of(kw))


def check_margins():
    """the margin condition over every size and option set the tests use; the subsets of points and the first M images the tests
    take are subsets of what is checked here"""
    worst = dict(compare=np.inf, texel=np.inf)
    for size in range(len(cc.SIZES)):
        for kw in OPTION_SETS:
            m = expected(size, **kw)["margins"]
            worst = {k: min(worst[k], m[k]) for k in worst}
    assert worst["compare"] >= mc.MIN_MARGIN and worst["texel"] >= TEXEL_MARGIN, worst
    return worst


def turned(size, degrees, seed):
    """the first 18 cameras, each turned about its centre by a seeded rotation of `degrees` about a random axis, with the depth
    images re-rendered analytically at the turned cameras: (Rcw [18, 3, 3], tcw [18, 3], depth [18, H, W])"""
    s = scene(size)
    rng = np.random.default_rng(seed)
    N = cc.N_CAMERAS
    R = np.empty((N, 3, 3))
    for k in range(N):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = np.deg2rad(degrees)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R[k] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K) @ s["Rcw"][k]
    t = -np.einsum("nij,nj->ni", R, s["C"][:N])
    depth = np.stack([cc.analytic_depth(s["intr"], R[k], s["C"][k], s["W"], s["H"]) for k in range(N)])
    return np.ascontiguousarray(R), np.ascontiguousarray(t), np.ascontiguousarray(depth)


def constant_images(size, seed=5):
    """uint8 [21, H, W, 3]: image k one colour (b_k, g_k, r_k); and the colours int64 [21, 3]"""
    s = scene(size)
    colours = np.random.default_rng(seed).integers(0, 256, (cc.N_IMAGES, 3))
    colours[3] = 255
    colours[4] = 0
    img = np.broadcast_to(colours[:, None, None, :].astype(np.uint8), (cc.N_IMAGES, s["H"], s["W"], 3))
    return np.ascontiguousarray(img), colours.astype(np.int64)


def closed_form(seen, colours, min_views=2):
    """(n_views, S1, S2, rgb [n, 3] r g b, N [n, 3]) of constant-colour images from which images see a point: every sample is exactly
    256 colour, integer arithmetic written out here; sigma is sqrt(((N_b + N_g) + N_r) / (3 * 65536 n^2)) where n >= min_views"""
    seen = np.asarray(seen, np.int64)                                 # [M, n]
    n = seen.sum(0)
    S1 = 256 * (seen.T @ colours)
    S2 = 65536 * (seen.T @ (colours * colours))
    nn = np.maximum(n, 1)[:, None]
    rgb = np.where(n[:, None] > 0, (2 * S1 + 256 * nn) // (512 * nn), 0)[:, ::-1].astype(np.uint8)
    return n.astype(np.int32), S1.astype(np.uint32), S2, np.ascontiguousarray(rgb), n[:, None] * S2 - S1 * S1


def pixel_edge_case():
    """The pixel edges in exact arithmetic: R = I, t = 0, no distortion, fx = fy = 64, cx = cy = 32, points (x, y, 1) with dyadic
    x, y, so u = 64 x + 32 and v = 64 y + 32 are exact, and a 65 x 65 image in which every texel has its own value.  dict(points,
    image [1, 65, 65, 3], intr, u, v): u, v the exact pixel of every point (NaN for the two points that project nowhere)."""
    W = H = 65
    intr = np.array([64.0, 64.0, 32.0, 32.0, 0, 0, 0, 0])
    edge = [0.0, 1 / 256, 255 / 256, 1.0, 31.5, 63.0, 63 + 1 / 256, 63 + 255 / 256, 64 - 1 / 256, 64.0, 64.5, -1 / 256]
    uv = [(a, b) for a in edge for b in (0.0, 17 + 1 / 256, 63 + 255 / 256, 64.0)] + [(b, a) for a in edge for b in (5 + 255 / 256, 40.0)]
    uv = np.array(uv)
    pts = np.concatenate([np.stack([(uv[:, 0] - 32) / 64, (uv[:, 1] - 32) / 64, np.ones(len(uv))], 1),
                          [[0.25, 0.25, 0.0], [0.25, 0.25, -1.0]]]).astype(np.float32)      # Z = 0 and behind the camera
    assert (pts[:-2, :2].astype(np.float64) * 64 + 32 == uv).all()                             # dyadic: exact in float
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    idx = yy * W + xx                                                 # (b, g) alone tell the texels apart
    image = np.stack([idx % 256, (idx // 256) * 13 + 7, (37 * xx + 91 * yy) % 256], 2).astype(np.uint8)
    return dict(points=np.ascontiguousarray(pts), image=np.ascontiguousarray(image[None]), intr=intr, W=W, H=H,
                u=np.concatenate([uv[:, 0], [np.nan, np.nan]]), v=np.concatenate([uv[:, 1], [np.nan, np.nan]]))
