"""Fixture of the co-visibility tests (tests/test_covis_host.py on the CPU, tests/test_gpu_covis.py on the GPU): a 12 x 12 x 3 m
room with a partition wall that leaves a door, cameras on a loop through the door and cameras that face the partition from both
sides, analytic depth images, and planted surface points whose true visibility is ray-cast.  Built at test time; nothing is
committed.  World axes are a camera's: x right, y down, z forward; a camera with yaw a looks along (sin a, 0, cos a).

Images: 0-13 the loop, 14-17 facing the partition, 18 a twin of camera 0 at the identical pose (tied scores for the cap), 19 a view
of its own with 70 % of its pixels zeroed at random (the ring search; not at another image's pose, where a sample found in column
0 would project onto column 0 of that image to within an ulp), 20 camera 9 again with an all-zero depth image (n = 0).

Margin condition (as in match_cases.py): the device divides in the projection, so the fixture must not hold a decision an ulp
could turn.  `check_margins` asserts that every evaluated in-image comparison and every Z against its occlusion bound is at least
match_cases.MIN_MARGIN (relative) away from the bound, for every shape and option set the tests use.  It is a condition on the
fixture, checked on the CPU, not a tolerance on the device.  Eligibility compares integers and correctly rounded quotients of
small integers and needs no margin."""
import functools
import importlib

import numpy as np

import covis_oracle as co
import match_cases as mc

SIZES = ((160, 128), (37, 29))                                      # the second: an odd stride
GRIDS = ((16, 12), (7, 5), (9, 8), (1, 1))                          # 192; 35 < one wavefront; 72 = one and a tail of 8; one
N_LOOP, N_CAMERAS, N_IMAGES = 14, 18, 21
TWIN, HOLES, EMPTY = 18, 19, 20
M_VALUES = (N_IMAGES, 2, 1)
HOLE_FRACTION = 0.7
HOLES_POSE = (-2.1, 0.05, 2.7, 2.2)                                 # x, y, z, yaw of image 19
N_PLANTED = 4200
# x0, x1, y0, y1, z0, z1 of the walls: x = +-6, z = +-6, floor and ceiling y = +-1.5, the partition x = 0 for z in [-6, 2]
RECTS = np.array([[-6, -6, -1.5, 1.5, -6, 6], [6, 6, -1.5, 1.5, -6, 6], [-6, 6, -1.5, 1.5, -6, -6], [-6, 6, -1.5, 1.5, 6, 6],
                  [-6, 6, -1.5, -1.5, -6, 6], [-6, 6, 1.5, 1.5, -6, 6], [0, 0, -1.5, 1.5, -6, 2]], np.float64)
# the option sets of lvba_covis_pairs the GPU tests run (on top of the shape's grid)
OPTION_SETS = (dict(), dict(occlusion=0), dict(both_ways=1), dict(max_per_image=1), dict(max_per_image=3),
               dict(max_per_image=1, both_ways=1), dict(max_per_image=1, occlusion=0), dict(min_shared=40), dict(min_shared=0, min_overlap=0.0),
               dict(min_overlap=0.3), dict(min_overlap=0.3, both_ways=1, max_per_image=3))


def intrinsics(W, H):
    """synth.REF_INTRINSICS scaled to the image size, distortion included"""
    synth = importlib.import_module("global-lvba_amd.synth")
    intr = np.array(synth.REF_INTRINSICS, np.float64)
    W0, H0 = synth.REF_IMAGE_WH
    intr[[0, 2]] *= W / W0
    intr[[1, 3]] *= H / H0
    return intr


def camera_poses():
    """(centres [19, 3], yaw [19]): the cameras and the view of the image with holes"""
    a = 2.0 * np.pi * np.arange(N_LOOP) / N_LOOP
    C = np.stack([3.2 * np.cos(a), 0.1 * np.sin(3 * a), 3.6 * np.sin(a) - 0.5], 1)
    yaw = np.arctan2(-3.2 * np.sin(a), 3.6 * np.cos(a))              # along the tangent
    C = np.vstack([C, [[-3, 0, -3.5], [-3, 0, -0.5], [3, 0, -3.5], [3, 0, -0.5]], [HOLES_POSE[:3]]])
    yaw = np.concatenate([yaw, [np.pi / 2 + 0.3, np.pi / 2 - 0.3, -np.pi / 2 - 0.3, -np.pi / 2 + 0.3, HOLES_POSE[3]]])
    return C, yaw


def cast(origin, dirs):
    """the parameter of the nearest wall along origin + s dirs [n, 3] (inf where the ray meets none)"""
    best = np.full(len(dirs), np.inf)
    with np.errstate(all="ignore"):
        for x0, x1, y0, y1, z0, z1 in RECTS:
            lo, hi = np.array([x0, y0, z0]), np.array([x1, y1, z1])
            k = int(np.flatnonzero(lo == hi)[0])                     # the axis the rectangle is normal to
            s = (lo[k] - origin[k]) / dirs[:, k]
            p = origin + s[:, None] * dirs
            ok = (s > 1e-9) & np.isfinite(s)
            for a in range(3):
                if a != k:
                    ok &= (p[:, a] >= lo[a] - 1e-9) & (p[:, a] <= hi[a] + 1e-9)
            best = np.where(ok & (s < best), s, best)
    return best


def analytic_depth(intr, Rcw, C, W, H):
    """float32 [H, W]: the camera-frame Z of the nearest wall along the undistorted ray of every pixel"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y, ok = co.undistort(intr, u.ravel(), v.ravel())
    assert ok.all()
    s = cast(C, np.stack([x, y, np.ones_like(x)], 1) @ Rcw)          # R^T r; the ray has Z = 1, so the parameter is the depth
    return np.where(np.isfinite(s), s, 0).astype(np.float32).reshape(H, W)


def planted_points(rng):
    """points on the walls, by area; a point on the partition is a point of both rooms, as the depth images see it"""
    area = np.array([(r[1] - r[0] or 1) * (r[3] - r[2] or 1) * (r[5] - r[4] or 1) for r in RECTS])
    which = rng.choice(len(RECTS), N_PLANTED, p=area / area.sum())
    lo, hi = RECTS[which][:, [0, 2, 4]], RECTS[which][:, [1, 3, 5]]
    return lo + rng.uniform(0.02, 0.98, (N_PLANTED, 3)) * (hi - lo)


def visible(P, intr, Rcw, tcw, C, W, H):
    """bool [n]: the planted point projects into the image and the ray from the camera meets no wall before it"""
    u, v, _, ok = co.project(intr, Rcw, tcw, P)
    ok = ok & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    d = P - C
    return ok & (cast(C, d) >= 1.0 - 1e-6)                           # the parameter of the point itself is 1


@functools.lru_cache(None)
def room(size=0):
    """dict(depth [21, H, W], intr, Rcw [21, 3, 3], tcw [21, 3], W, H, vis [18, n_planted] the planted points' true visibility)"""
    W, H = SIZES[size]
    rng = np.random.default_rng(2027 + size)
    intr = intrinsics(W, H)
    C, yaw = camera_poses()
    Rcw = np.stack([mc._rot(0.0, a, 0.0).T for a in yaw])
    tcw = -np.einsum("nij,nj->ni", Rcw, C)
    depth = np.stack([analytic_depth(intr, Rcw[k], C[k], W, H) for k in range(N_CAMERAS + 1)])
    P = planted_points(rng)
    vis = np.stack([visible(P, intr, Rcw[k], tcw[k], C[k], W, H) for k in range(N_CAMERAS)])
    order = list(range(N_CAMERAS)) + [0, N_CAMERAS, 9]               # + the twin, the image with holes, the empty image
    Rcw, tcw, depth = Rcw[order], tcw[order], depth[order]
    depth[HOLES][rng.uniform(size=depth[HOLES].shape) < HOLE_FRACTION] = 0
    depth[EMPTY] = 0
    assert len(depth) == N_IMAGES
    return dict(depth=np.ascontiguousarray(depth), intr=intr, Rcw=np.ascontiguousarray(Rcw), tcw=np.ascontiguousarray(tcw), W=W, H=H,
                vis=vis, planted=P)


def grid_opts(grid):
    return dict(grid_x=GRIDS[grid][0], grid_y=GRIDS[grid][1])


@functools.lru_cache(None)
def lifted(size, grid, M=N_IMAGES):
    """(world [M, G, 3], ring [M, G]) of the first M images"""
    r = room(size)
    return co.samples(r["depth"][:M], r["intr"], r["Rcw"][:M], r["tcw"][:M], **grid_opts(grid))


@functools.lru_cache(None)
def judged(size, grid, occlusion, M=N_IMAGES):
    """(fate [M, M, G], margin, n_points [M], counts [M, M]) of the first M images"""
    r = room(size)
    world, _ = lifted(size, grid, M)
    fate, margin = co.fates(r["depth"][:M], r["intr"], r["Rcw"][:M], r["tcw"][:M], world, with_margin=True, occlusion=occlusion)
    return (fate, margin) + co.counts(fate, world)


def selected(size, grid, M=N_IMAGES, **kw):
    """(pairs, score, shared) of the oracle"""
    _, _, n, c = judged(size, grid, dict(co.DEFAULTS, **kw)["occlusion"], M)
    return co.select(n, c, **kw)


def check_margins():
    """the margin condition over every shape the tests use (the option sets differ in the occlusion switch alone, as far as a
    floating-point comparison goes)"""
    worst = np.inf
    for size in range(len(SIZES)):
        for grid in range(len(GRIDS)):
            for occlusion in (0, 1):
                for M in M_VALUES:
                    worst = min(worst, judged(size, grid, occlusion, M)[1])
    assert worst >= mc.MIN_MARGIN, worst
    return worst


def shared_planted(size=0):
    """int [18, 18]: the planted points both cameras see"""
    v = room(size)["vis"].astype(np.int64)
    return v @ v.T
