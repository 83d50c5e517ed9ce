"""Fixture of the depth-guided gate's tests (tests/test_match_depth_host.py on the CPU, tests/test_gpu_match_depth.py on the GPU):
views of a slanted facade whose textures repeat ALONG the epipolar lines of three cameras on a horizontal baseline, analytic depth
images with holes, and the keypoint counts at which the scan kernel changes path.  Built at test time; nothing is committed.

Margin condition (as in match_cases.py): the device divides in the projection and evaluates acos with its own libm, so the fixture
must not hold a decision an ulp could turn.  `check_margins` asserts that every evaluated |d^2 - rho^2| / rho^2 and every acos
clause is at least match_cases.MIN_MARGIN away from its bound, for every option set the tests use.  It is a condition on the
fixture, checked on the CPU, not a tolerance on the device.  A distance that is infinite (a prediction that is nowhere) or NaN (a
NaN pixel) fails exactly and carries no margin."""
import functools
import importlib

import numpy as np

import match_cases as mc
import match_depth_oracle as mdo
import match_oracle as mo

PLANE_Z0, PLANE_SLOPE = 8.0, 0.15                                  # the facade: z = 8 + 0.15 x
N_TEX, N_COPIES, N_UNIQUE = 12, 5, 80
N_REP = N_TEX * N_COPIES
# per image: the keypoint count.  0-2: the horizontal baseline; 3: off it; 4: a close-up in front of the others (a point lifted
# 3 m before view 0 lies behind it); 5: one keypoint; 6: none.  300: three workgroups of rows; 129: one row into the second
# workgroup; 161, 33, 31: either side of a 32-column tile.
COUNTS = (300, 129, 161, 33, 31, 1, 0)
DISTRACTORS = (160, 8, 8, 4, 4, 0, 0)                               # at least: an image with fewer visible points gets more
CENTRES = np.array([[0, 0, 0], [0.55, 0, 0], [-0.5, 0, 0], [0.2, -0.6, 0.3], [0.1, 0.3, 3.5], [0.3, 0.2, 0.1], [0, 0.4, 0]], np.float64)
ANGLES = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0.05, 0.04, -0.03], [-0.03, 0.02, 0.04], [0.01, -0.02, 0], [0, 0, 0]], np.float64)
HOLES = {0: (250, 150, 420, 330), 1: (170, 240, 330, 420)}         # view: (u0, v0, u1, v1) zeroed, [u0, u1) x [v0, v1)
POLE = (60, 60, 68, 68, 3.0)                                       # view 0: a patch 3 m away
DEPTH_OPTION_SETS = (dict(guided=2), dict(guided=2, mutual=0), dict(guided=2, max_reproj_px=3))
PAIRS = np.array([(0, 1), (0, 2), (1, 2), (0, 3), (3, 1), (2, 3), (0, 4), (4, 3), (5, 0), (1, 5), (6, 0), (2, 6), (5, 6), (4, 1)], np.int32)
HORIZONTAL = ((0, 1), (0, 2), (1, 2))


def plane_depth(intr, R, t, W, H):
    """float32 [H, W]: the camera-frame Z of the facade along the ray of every pixel centre (0 where the ray misses it)"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd, yd
    for _ in range(8):
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * r2 * r2
        x, y = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / radial, (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / radial
    n, c = np.array([-PLANE_SLOPE, 0.0, 1.0]), PLANE_Z0              # n . X = c
    ray = np.stack([x, y, np.ones_like(x)], -1) @ R                   # R^T r
    s = (c + n @ (R.T @ t)) / (ray @ n)
    return np.where(s > 0, s, 0).astype(np.float32)


@functools.lru_cache(None)
def facade():
    """dict(descs, keypoints, depth [7, H, W], intr, Rcw, tcw, Rcw2, tcw2, point (the 3-D point of every keypoint, -1: none),
    X, special (image, keypoint) of the NaN pixel, the pole keypoint and the keypoint on the hole's edge)"""
    synth = importlib.import_module("global-lvba_amd.synth")
    import torch
    rng = np.random.default_rng(2026)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    W, H = synth.REF_IMAGE_WH
    rows = np.linspace(-2.0, 2.0, N_TEX)
    xs = np.concatenate([-1.6 + 0.8 * np.arange(N_COPIES) + 0.07 * ((k * 5) % 7 - 3) for k in range(N_TEX)])
    X = np.zeros((N_REP + N_UNIQUE, 3))
    X[:N_REP, 0], X[:N_REP, 1] = xs, np.repeat(rows, N_COPIES)       # texture k: points 5 k .. 5 k + 4, one row of constant y
    X[N_REP:, 0], X[N_REP:, 1] = rng.uniform(-2.4, 2.4, N_UNIQUE), rng.uniform(-2.2, 2.2, N_UNIQUE)
    X[:, 2] = PLANE_Z0 + PLANE_SLOPE * X[:, 0]
    tex = mc.sift_like(rng, N_REP + N_UNIQUE)
    tex[:N_REP] = tex[np.repeat(np.arange(N_TEX), N_COPIES)]
    Rcw = np.stack([mc._rot(*a) for a in ANGLES])
    tcw = -np.einsum("nij,nj->ni", Rcw, CENTRES)
    depth = np.stack([plane_depth(intr, Rcw[v], tcw[v], W, H) for v in range(len(COUNTS))])
    for v, (u0, v0, u1, v1) in HOLES.items():
        depth[v, v0:v1, u0:u1] = 0
    depth[0, POLE[1]:POLE[3], POLE[0]:POLE[2]] = POLE[4]
    descs, kps, point = [], [], []
    for v, n in enumerate(COUNTS):
        uv = synth.project_distorted(torch.from_numpy(X @ Rcw[v].T + tcw[v]), intr).numpy() + rng.normal(0, 0.3, (len(X), 2))
        inside = np.flatnonzero((uv[:, 0] > 2) & (uv[:, 0] < W - 3) & (uv[:, 1] > 2) & (uv[:, 1] < H - 3))
        rep, uniq = inside[inside < N_REP], rng.permutation(inside[inside >= N_REP])
        cand = np.concatenate([rep, uniq]) if v < 3 else rng.permutation(inside)     # the baseline views keep every repeated point
        idx = rng.permutation(cand[:n - DISTRACTORS[v]])
        n_dis = n - len(idx)
        d = np.vstack([mc.noisy(rng, tex[idx], 6), mc.sift_like(rng, n_dis)]) if n else np.zeros((0, 128), np.uint8)
        k = np.vstack([uv[idx], np.stack([rng.uniform(2, W - 3, n_dis), rng.uniform(2, H - 3, n_dis)], 1)]).astype(np.float32)
        descs.append(np.ascontiguousarray(d)); kps.append(k.reshape(-1, 2))
        point.append(np.concatenate([idx, np.full(n_dis, -1)]).astype(np.int64))
    # special keypoints, all distractors (the last rows of their image)
    kps[1][-1] = np.nan                                                # a NaN pixel: no point, and no distance to it
    kps[0][-1] = (POLE[0] + 3.4, POLE[1] + 2.7)                        # lifted 3 m before view 0: behind view 4, nowhere there
    kps[0][-2] = (HOLES[0][0] - 0.5, HOLES[0][1] - 0.5)                # three valid neighbours, the fourth in the hole: no point
    special = dict(nan=(1, COUNTS[1] - 1), pole=(0, COUNTS[0] - 1), edge=(0, COUNTS[0] - 2))
    Rcw2, tcw2 = Rcw.copy(), tcw.copy()                                # a trajectory update of view 1
    Rcw2[1] = mc._rot(0.004, -0.003, 0.002) @ Rcw[1]
    tcw2[1] = tcw[1] + np.array([0.05, -0.02, 0.01])
    return dict(descs=descs, keypoints=kps, depth=depth, intr=intr, Rcw=Rcw, tcw=tcw, Rcw2=Rcw2, tcw2=tcw2, point=point, X=X,
                special=special, n_repeated=N_REP, pairs=PAIRS)


@functools.lru_cache(None)
def geometry(second=False):
    f = facade()
    return mdo.DepthGeometry(f["keypoints"], f["intr"], f["Rcw2" if second else "Rcw"], f["tcw2" if second else "tcw"], f["depth"])


def pair_margin(descs, a, b, geom, **kw):
    """the smallest margin of any decision of the ordered pair (a, b) that is not exact: the acos clauses of match_cases.py and
    the gate's distances"""
    o = dict(mdo.DEFAULTS, **kw)
    best, s1, s2 = mdo.scan(descs, a, b, geom, **o)
    d1, d2 = mo.distance(s1), mo.distance(s2)
    has = best >= 0
    inexact = has & ~((s1 >= 262144) & (s2 >= 262144))
    m = np.inf
    if has.any():
        m = min(m, np.abs(d1[has] - o["max_distance"]).min())
    if inexact.any():
        m = min(m, np.abs(d1[inexact] - o["max_ratio"] * d2[inexact]).min())
    if o["guided"] == 2:
        m = min(m, geom.depth_mask(a, b, o["max_reproj_px"], with_margin=True)[1])
    elif o["guided"] == 1:
        m = min(m, geom.mask(a, b, o["max_epipolar_px"], with_margin=True)[1])
    return m


def check_margins(descs, pairs, option_sets, geom):
    worst = np.inf
    for kw in option_sets:
        for a, b in np.asarray(pairs).reshape(-1, 2):
            for x, y in ((a, b), (b, a)):
                worst = min(worst, pair_margin(descs, int(x), int(y), geom, **kw))
    assert worst >= mc.MIN_MARGIN, worst
    return worst
