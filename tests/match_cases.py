"""Fixtures of the descriptor matcher's tests (tests/test_match_host.py on the CPU, tests/test_gpu_match.py on the GPU): SIFT-like
descriptors with planted correspondences, the edge cases of the top-two rule, and a synthetic multi-view set for the guided gate.

Margin condition: the device evaluates acos and the three fp64 clauses with its own libm, so a fixture must not hold a decision
that an ulp could turn.  Every case reports the smallest oracle margin of any decision -- |d1 - max_distance|,
|d1 - max_ratio d2|, and under the gate |e^2 - bound| / bound -- and `check_margins` asserts none is under 1e-9.  This is a
condition on the fixtures, checked on the CPU; it is not a tolerance on the device.  Two kinds of decision are exact and carry
no margin: a ratio clause whose two scores are both clamped (s >= 262144 gives d = acos(1) = 0 on any libm, and 0 < 0 is false),
and the gate of a pair without epipolar geometry (E = 0: 0 <= 0)."""
import functools
import importlib

import numpy as np

import match_oracle as mo

MIN_MARGIN = 1e-9


def sift_like(rng, n):
    """gamma-distributed bins, clipped at 0.2, renormalised, x 512 rounded"""
    d = rng.gamma(0.6, 1.0, (n, 128))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.minimum(d, 0.2)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.minimum(np.floor(512 * d + 0.5), 255).astype(np.uint8)


def noisy(rng, d, sigma):
    """a re-observation of descriptors d"""
    x = np.maximum(d.astype(np.float64) + rng.normal(0, sigma, d.shape), 0)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.minimum(np.floor(512 * x + 0.5), 255).astype(np.uint8)


# ---- unguided ---------------------------------------------------------------------------------------------------------------------
# sizes: nothing, one (the s2 = 0 branch), either side of the 32-row / 32-column tile, of the 128-row workgroup, and one image of
# about 1000 (several workgroups, dozens of column tiles per row)
SIZES = (0, 1, 31, 32, 33, 64, 70, 129, 257, 1003)
# per image the noise of its re-observation: low (everything passes), medium (the ratio test rejects), high (the distance bound
# rejects)
NOISE = (12, 12, 12, 30, 12, 60, 12, 30, 12, 30)
OPTION_SETS = (dict(), dict(mutual=0), dict(max_distance=1.2, max_ratio=0.97), dict(max_distance=0.45, max_ratio=0.6, mutual=0))


@functools.lru_cache(None)
def unguided():
    """dict(descs, pairs, planted): planted[i] = the landmark of every descriptor of image i (-1: a distractor)"""
    rng = np.random.default_rng(20260417)
    pool = sift_like(rng, 700)
    descs, planted = [], []
    for n, s in zip(SIZES, NOISE):
        shared = (2 * n) // 3 if n > 1 else n
        lm = rng.choice(len(pool), shared, replace=False)
        d = np.vstack([noisy(rng, pool[lm], s), sift_like(rng, n - shared)]) if n else np.zeros((0, 128), np.uint8)
        p = rng.permutation(n)
        descs.append(np.ascontiguousarray(d[p]))
        planted.append(np.concatenate([lm, np.full(n - shared, -1)])[p].astype(np.int64))
    # the edge images
    base = descs[6]                                                   # 70 descriptors
    dup_b = base.copy(); dup_b[41] = dup_b[7]; dup_b[55] = dup_b[7]   # exact duplicates among the columns: tie -> lowest, s2 = s1
    dup_a = noisy(rng, base, 8); dup_a[50] = dup_a[3]                 # exact duplicates among the rows: mutual keeps the lower
    extreme = noisy(rng, base[:40], 8)
    extreme[5] = 0; extreme[6] = 255; extreme[7] = 3; extreme[8] = 200; extreme[9, :64] = 255; extreme[9, 64:] = 0
    descs += [dup_b, dup_a, extreme]
    planted += [np.full(len(x), -1, np.int64) for x in (dup_b, dup_a, extreme)]
    n_img = len(descs)
    DUP_B, DUP_A, EXT = n_img - 3, n_img - 2, n_img - 1
    pairs = [(8, 9), (9, 8), (7, 8), (2, 4), (4, 2), (3, 5), (5, 7), (1, 6), (6, 1), (0, 6), (6, 0), (1, 0), (9, 5), (3, 9), (2, 3),
             (6, DUP_B), (DUP_B, 6), (DUP_A, 6), (6, DUP_A), (DUP_A, DUP_B), (EXT, 6), (6, EXT), (EXT, DUP_B), (9, 2), (4, 9)]
    return dict(descs=descs, pairs=np.array(pairs, np.int32), planted=planted, DUP_B=DUP_B, DUP_A=DUP_A, EXT=EXT)


def pair_margin(descs, a, b, geom=None, **kw):
    """the smallest margin of any decision of the ordered pair (a, b) that is not exact (see the module's text)"""
    o = dict(mo.DEFAULTS, **kw)
    best, s1, s2 = mo.scan(descs, a, b, geom, **o)
    d1, d2 = mo.distance(s1), mo.distance(s2)
    has = best >= 0
    inexact = has & ~((s1 >= 262144) & (s2 >= 262144))
    m = np.inf
    if has.any():
        m = min(m, np.abs(d1[has] - o["max_distance"]).min())
    if inexact.any():
        m = min(m, np.abs(d1[inexact] - o["max_ratio"] * d2[inexact]).min())
    if o["guided"]:
        m = min(m, geom.mask(a, b, o["max_epipolar_px"], with_margin=True)[1])
    return m


def check_margins(descs, pairs, option_sets, geom=None):
    worst = np.inf
    for kw in option_sets:
        for a, b in np.asarray(pairs).reshape(-1, 2):
            for x, y in ((a, b), (b, a)):
                worst = min(worst, pair_margin(descs, int(x), int(y), geom, **kw))
    assert worst >= MIN_MARGIN, worst
    return worst


def rejections(descs, pairs, geom=None, **kw):
    """how many rows with a best column each clause turns away: (distance, ratio, mutual)"""
    o = dict(mo.DEFAULTS, **kw)
    nd = nr = nm = 0
    for a, b in np.asarray(pairs).reshape(-1, 2):
        best, s1, s2 = mo.scan(descs, int(a), int(b), geom, **o)
        back = mo.scan(descs, int(b), int(a), geom, **o)[0]
        if not len(back):
            continue
        d1, d2 = mo.distance(s1), mo.distance(s2)
        has = best >= 0
        nd += int((has & ~(d1 < o["max_distance"])).sum())
        nr += int((has & (d1 < o["max_distance"]) & ~(d1 < o["max_ratio"] * d2)).sum())
        nm += int((has & (d1 < o["max_distance"]) & (d1 < o["max_ratio"] * d2) & (back[np.maximum(best, 0)] != np.arange(len(best)))).sum())
    return nd, nr, nm


# ---- guided -----------------------------------------------------------------------------------------------------------------------
GUIDED_OPTION_SETS = (dict(guided=1), dict(guided=1, mutual=0), dict(guided=1, max_epipolar_px=1.5))


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@functools.lru_cache(None)
def guided():
    """Four views of 150 points (the first 60 are 15 textures repeated at 4 different points each), a fifth view at the pose of
    view 0 (no epipolar geometry against it), one keypoint whose undistortion fails.  dict(descs, keypoints, intr, Rcw, tcw, Rcw2,
    tcw2 (other poses), pairs, point (the 3-D point of every keypoint), n_repeated)."""
    synth = importlib.import_module("global-lvba_amd.synth")
    import torch
    rng = np.random.default_rng(515)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    W, H = synth.REF_IMAGE_WH
    n_rep, n_pts = 60, 150
    X = np.stack([rng.uniform(-3.0, 3.0, n_pts), rng.uniform(-2.2, 2.2, n_pts), rng.uniform(6.0, 11.0, n_pts)], 1)
    tex = sift_like(rng, n_pts)
    tex[:n_rep] = tex[np.arange(n_rep) % 15]                        # texture k at points k, k + 15, k + 30, k + 45
    centres = np.array([[0, 0, 0], [0.9, 0.1, 0.05], [-0.7, 0.5, 0.2], [0.3, -0.8, -0.1], [0, 0, 0]], np.float64)
    angles = np.array([[0, 0, 0], [0.02, -0.08, 0.03], [-0.04, 0.07, -0.02], [0.06, 0.03, 0.05], [0, 0, 0]], np.float64)
    Rcw = np.stack([_rot(*a) for a in angles])
    tcw = -np.einsum("nij,nj->ni", Rcw, centres)
    descs, kps, point = [], [], []
    for v in range(len(Rcw)):
        Xc = X @ Rcw[v].T + tcw[v]
        uv = synth.project_distorted(torch.from_numpy(Xc), intr).numpy()
        uv = uv + rng.normal(0, 0.3, uv.shape)
        inside = (uv[:, 0] > 2) & (uv[:, 0] < W - 2) & (uv[:, 1] > 2) & (uv[:, 1] < H - 2)
        idx = np.flatnonzero(inside)
        idx = idx[rng.permutation(len(idx))]
        n_dis = 12
        d = np.vstack([noisy(rng, tex[idx], 6), sift_like(rng, n_dis)])
        k = np.vstack([uv[idx], np.stack([rng.uniform(2, W - 2, n_dis), rng.uniform(2, H - 2, n_dis)], 1)]).astype(np.float32)
        descs.append(np.ascontiguousarray(d)); kps.append(k)
        point.append(np.concatenate([idx, np.full(n_dis, -1)]).astype(np.int64))
    kps[1][int(np.flatnonzero(point[1] >= n_rep)[0])] = np.nan      # a keypoint whose undistortion fails
    # other poses for a second set_geometry: view 1 turned and moved by what a trajectory update might do
    Rcw2, tcw2 = Rcw.copy(), tcw.copy()
    Rcw2[1] = _rot(0.004, -0.003, 0.002) @ Rcw[1]
    tcw2[1] = tcw[1] + np.array([0.05, -0.02, 0.01])
    pairs = np.array([(0, 1), (1, 0), (0, 2), (1, 2), (3, 1), (2, 3), (0, 3), (0, 4), (4, 1)], np.int32)
    return dict(descs=descs, keypoints=kps, intr=intr, Rcw=Rcw, tcw=tcw, Rcw2=Rcw2, tcw2=tcw2, pairs=pairs, point=point,
                n_repeated=n_rep, X=X)


def guided_geometry(second=False):
    g = guided()
    return mo.Geometry(g["keypoints"], g["intr"], g["Rcw2" if second else "Rcw"], g["tcw2" if second else "tcw"])


def planted_matches(g, a, b, repeated=None):
    """the (r, c) of the ordered pair (a, b) that observe the same 3-D point; repeated: True / False restricts to the repeated /
    the unique textures"""
    pa, pb = g["point"][a], g["point"][b]
    where = {int(p): c for c, p in enumerate(pb) if p >= 0}
    out = [(r, where[int(p)]) for r, p in enumerate(pa)
           if p >= 0 and int(p) in where and (repeated is None or (p < g["n_repeated"]) == repeated)]
    return set(out)
