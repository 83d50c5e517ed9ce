"""Fixtures of the two-view verification's tests (tests/test_verify_host.py on the CPU, tests/test_gpu_verify.py on the GPU): 3-D
points in front of four cameras with the repository's usual intrinsics (non-zero distortion), keypoints with 0.3 px of noise, and
per image pair a list of putative matches with a stated share of outliers, each at least 20 px off its epipolar line in both
images under the true E.  One scene in general position, one that is a single slanted plane.  The true poses are kept.

Margin condition: the device and the oracle form a hypothesis from the same operations in the same order, so their E agree to
the bit; what is asserted on top (test_verify_host.py) is that no inlier decision of any (fixture, hypothesis, match) the GPU
tests use has its two sides within 1e-9 relative of each other -- a condition on the fixtures, not a tolerance on the device."""
import functools
import importlib

import numpy as np

import match_oracle as mo
import verify_oracle as vo
from match_cases import _rot

MIN_MARGIN = 1e-9
CHUNK = 1024                      # verify.hip's VERIFY_CHUNK
HB = 64                           # ransac_batch.h's RANSAC_HB
SIZES0 = (0, 7, 8, 9, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1)
SIZES1 = (0, 1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1)
H_SMALL = 200                     # not a multiple of HB: the last block of a pair is partly idle
H_EDGES = (1, 63, 64, 65)
IMAGE_PAIRS = ((0, 1), (0, 2), (1, 2), (3, 1), (2, 3), (0, 3), (2, 0))   # two of them given as (hi, lo)
N_POINTS, N_EXTRA = 1300, 300
OUTLIER_PX = 20.0


def _scene(planar, seed):
    synth = importlib.import_module("global-lvba_amd.synth")
    import torch
    rng = np.random.default_rng(seed)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    W, Hh = synth.REF_IMAGE_WH
    x, y = rng.uniform(-2.6, 2.6, N_POINTS), rng.uniform(-2.0, 2.0, N_POINTS)
    z = 8.0 + 0.45 * x - 0.3 * y if planar else rng.uniform(6.0, 11.0, N_POINTS)
    X = np.stack([x, y, z], 1)
    centres = np.array([[0, 0, 0], [0.9, 0.1, 0.05], [-0.7, 0.5, 0.2], [0.3, -0.8, -0.1]], np.float64)
    angles = np.array([[0, 0, 0], [0.02, -0.08, 0.03], [-0.04, 0.07, -0.02], [0.06, 0.03, 0.05]], np.float64)
    Rcw = np.stack([_rot(*a) for a in angles])
    tcw = -np.einsum("nij,nj->ni", Rcw, centres)
    kps = []
    for v in range(4):
        uv = synth.project_distorted(torch.from_numpy(X @ Rcw[v].T + tcw[v]), intr).numpy()
        uv = uv + rng.normal(0, 0.3, uv.shape)
        extra = np.stack([rng.uniform(2, W - 2, N_EXTRA), rng.uniform(2, Hh - 2, N_EXTRA)], 1)
        kps.append(np.vstack([uv, extra]).astype(np.float32))
    kps[1][N_POINTS - 3:N_POINTS] = np.nan          # three keypoints of image 1 whose undistortion fails
    xy = [mo.undistort_all(intr, k) for k in kps]
    return dict(keypoints=kps, xy=xy, intr=intr, Rcw=Rcw, tcw=tcw, X=X, rng_seed=seed)


def true_E(sc, a, b):
    lo, hi = min(a, b), max(a, b)
    return mo.essential(sc["Rcw"][lo], sc["tcw"][lo], sc["Rcw"][hi], sc["tcw"][hi]).reshape(9)


def line_distances_px(sc, a, b, matches):
    """the distance of each match's keypoints from the other's epipolar line under the true E, in pixels, (in lo, in hi)"""
    P = vo.points(sc["xy"], a, b, matches)
    E = true_E(sc, a, b).reshape(3, 3)
    xl = np.concatenate([P[:, :2], np.ones((len(P), 1))], 1)
    xh = np.concatenate([P[:, 2:], np.ones((len(P), 1))], 1)
    l, lt = xl @ E.T, xh @ E
    r = np.abs(np.einsum("ij,ij->i", xh, l))
    f = 0.5 * (sc["intr"][0] + sc["intr"][1])
    with np.errstate(invalid="ignore"):
        return f * r / np.hypot(lt[:, 0], lt[:, 1]), f * r / np.hypot(l[:, 0], l[:, 1])


def make_matches(sc, a, b, m, outlier_share, rng, with_nan=False):
    """(matches int32 [m, 2], planted bool [m]): planted matches join the two keypoints of one 3-D point"""
    n_out = int(round(outlier_share * m))
    n_in = m - n_out
    pts = rng.choice(N_POINTS - 3, n_in, replace=False)
    rows = [np.stack([pts, pts], 1)]
    out = np.zeros((0, 2), np.int64)
    while len(out) < n_out:
        cand = np.stack([rng.integers(0, N_POINTS + N_EXTRA, 4 * n_out + 8), rng.integers(0, N_POINTS + N_EXTRA, 4 * n_out + 8)], 1)
        dl, dh = line_distances_px(sc, a, b, cand)
        out = np.vstack([out, cand[(dl >= OUTLIER_PX) & (dh >= OUTLIER_PX) & (cand[:, 0] != cand[:, 1])]])
    rows.append(out[:n_out])
    mm = np.vstack(rows)
    planted = np.arange(m) < n_in
    if with_nan and m >= 12:                        # matches on the keypoints of image 1 that do not undistort
        col = 0 if a == 1 else 1
        for k in range(3):
            mm[n_in - 1 - k, col] = N_POINTS - 3 + k
            planted[n_in - 1 - k] = False
    p = rng.permutation(m)
    return np.ascontiguousarray(mm[p].astype(np.int32)), planted[p]


def _case(sc, name, a, b, matches, planted, **opts):
    return dict(name=name, a=int(a), b=int(b), matches=matches, planted=planted, opts=opts)


@functools.lru_cache(None)
def general():
    """dict(scene, claims, sizes0, sizes1, h_edges, special, flipped)"""
    sc = _scene(False, 20261019)
    rng = np.random.default_rng(77)
    claims = [_case(sc, "general-30%", 0, 1, *make_matches(sc, 0, 1, 300, 0.3, rng), method=0),
              _case(sc, "general-60%-rotation", 0, 2, *make_matches(sc, 0, 2, 300, 0.6, rng), method=1),
              _case(sc, "general-30%-nan", 3, 1, *make_matches(sc, 3, 1, 200, 0.3, rng, with_nan=True), method=0),
              _case(sc, "general-50%-nan-rotation", 1, 2, *make_matches(sc, 1, 2, 200, 0.5, rng, with_nan=True), method=1)]
    sizes = {}
    for method, ms in ((0, SIZES0), (1, SIZES1)):
        sizes[method] = [_case(sc, f"m={m}", *IMAGE_PAIRS[k % len(IMAGE_PAIRS)],
                               *make_matches(sc, *IMAGE_PAIRS[k % len(IMAGE_PAIRS)], m, 0.3, rng), method=method, hypotheses=H_SMALL)
                         for k, m in enumerate(ms)]
    # a mixed batch: every size above and more, about 40 pairs in one call
    mixed = {}
    for method, ms in ((0, SIZES0), (1, SIZES1)):
        extra = [int(x) for x in rng.integers(10, 400, 30)]
        mixed[method] = [_case(sc, f"mixed-{k}", *IMAGE_PAIRS[(k + 3) % len(IMAGE_PAIRS)],
                               *make_matches(sc, *IMAGE_PAIRS[(k + 3) % len(IMAGE_PAIRS)], m, 0.3, rng, with_nan=k % 5 == 0),
                               method=method, hypotheses=H_SMALL)
                         for k, m in enumerate(list(ms) + extra)]
    same = np.tile(np.array([[5, 5]], np.int32), (40, 1))       # every match the same match
    special = [_case(sc, "one-match-repeated", 0, 1, same, np.zeros(40, bool), method=0, hypotheses=H_SMALL),
               _case(sc, "one-match-repeated-rotation", 0, 1, same, np.zeros(40, bool), method=1, hypotheses=H_SMALL)]
    m65 = make_matches(sc, 0, 1, 65, 0.3, rng)
    h_edges = [_case(sc, f"H={H}-method{method}", 0, 1, *m65, method=method, hypotheses=H) for H in H_EDGES for method in (0, 1)]
    fm, fp = make_matches(sc, 1, 3, 150, 0.3, rng)
    flipped = [_case(sc, "lo-hi", 1, 3, fm, fp, method=0, hypotheses=H_SMALL),
               _case(sc, "hi-lo", 3, 1, np.ascontiguousarray(fm[:, ::-1]), fp, method=0, hypotheses=H_SMALL)]
    return dict(scene=sc, claims=claims, sizes=sizes, mixed=mixed, special=special, h_edges=h_edges, flipped=flipped)


@functools.lru_cache(None)
def planar():
    """the scene that is one plane: dict(scene, claims); the first claim is the rotation-aided method's, the second documents the
    eight-point method on the same matches"""
    sc = _scene(True, 20261020)
    rng = np.random.default_rng(79)       # 78 plants an outlier that a two-point model 25 px off the truth still takes in
    mm = make_matches(sc, 0, 1, 400, 0.6, rng)
    return dict(scene=sc, claims=[_case(sc, "planar-60%-rotation", 0, 1, *mm, method=1), _case(sc, "planar-60%-eight", 0, 1, *mm, method=0)])


def relative_rotation(sc, a, b):
    return vo.relative_rotation(sc["Rcw"][min(a, b)], sc["Rcw"][max(a, b)])


def options(sc, case, **over):
    return dict(vo.DEFAULTS, intr=sc["intr"], **dict(case["opts"], **over))


def case_points(sc, case):
    return vo.points(sc["xy"], case["a"], case["b"], case["matches"])


_ORACLE = {}


def oracle_hypotheses(sc, case, **over):
    """(E, count, idx, margin) of the case, computed once and shared"""
    o = options(sc, case, **over)
    key = (sc["rng_seed"], case["name"], case["a"], case["b"], tuple(sorted((k, v) for k, v in o.items() if k != "intr")))
    if key not in _ORACLE:
        lo, hi = min(case["a"], case["b"]), max(case["a"], case["b"])
        _ORACLE[key] = vo.hypotheses(case_points(sc, case), lo, hi, relative_rotation(sc, lo, hi), with_margin=True, **o)
    return _ORACLE[key]


_PAIR = {}


def oracle_pair(sc, case, **over):
    o = options(sc, case, **over)
    key = (sc["rng_seed"], case["name"], case["a"], case["b"], tuple(sorted((k, v) for k, v in o.items() if k != "intr")))
    if key not in _PAIR:
        lo, hi = min(case["a"], case["b"]), max(case["a"], case["b"])
        _PAIR[key] = vo.verify_pair(case_points(sc, case), lo, hi, relative_rotation(sc, lo, hi), **o)
    return _PAIR[key]


def all_gpu_cases():
    """every (scene, case) the GPU tests form hypotheses of"""
    g, p = general(), planar()
    out = [(g["scene"], c) for c in g["claims"] + g["sizes"][0] + g["sizes"][1] + g["mixed"][0] + g["mixed"][1] + g["special"] + g["h_edges"]
           + g["flipped"]]
    return out + [(p["scene"], c) for c in p["claims"]]
