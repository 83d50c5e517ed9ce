"""Fixture of the image front ends' shared pieces (tests/test_image_set_host.py on the CPU, tests/test_gpu_image_set.py on the GPU;
csrc/segments.h, csrc/image_set.h): ONE image set that the matcher, the verifier and the track builder all read, with key point
counts [0, 1, 0, 0, 65, 40, 0] -- empty images at both ends and two in a row, an image of one key point, an image longer than a
wavefront and than two 32-row scan tiles, an image of one tile and a part.  Built from the planar-facade machinery of
match_depth_cases.py (the facade z = 8 + 0.15 x, analytic depth images, textures with pixel and descriptor noise), so that the
depth lift is defined for every image.  Images 4 and 5 see the same 36 landmarks, image 4 nine more; image 1's single key point
is one of the shared ones; the rest are distractors without a landmark.  Built at test time; nothing is committed.

Margin condition, as in match_depth_cases.py and verify_cases.py: check_margins / hypothesis_margin assert on the CPU that no
fp64 decision of the oracles on this fixture is within 1e-9 of its bound.  A condition on the fixture, not a tolerance on the
device."""
import functools
import importlib

import numpy as np

import match_cases as mc
import match_depth_cases as mdc
import match_depth_oracle as mdo
import match_oracle as mo
import verify_oracle as vo

COUNTS = (0, 1, 0, 0, 65, 40, 0)
N_SHARED, N_ONLY4 = 36, 9
PAIRS = np.array([(0, 4), (4, 5), (5, 4), (1, 4), (2, 3), (6, 5)], np.int32)
VERIFY_PAIRS = np.array([(4, 5), (5, 4), (1, 4), (0, 4)], np.int32)
MATCH_OPTION_SETS = (dict(guided=0), dict(guided=1), dict(guided=2))
VERIFY_OPTION_SETS = (dict(method=0, hypotheses=200, refine_rounds=0), dict(method=1, hypotheses=200, refine_rounds=0))
THRESHOLDS = (2, 3)
CENTRES = np.array([[0, 0.4, 0], [-0.4, 0.1, 0], [0.2, 0.2, 0], [0.1, -0.3, 0.1], [0, 0, 0], [0.5, 0.05, 0.1], [-0.2, -0.2, 0]], np.float64)
ANGLES = np.array([[0, 0, 0], [0.01, -0.02, 0], [0, 0.01, 0], [0.02, 0, 0.01], [0, 0, 0], [0.02, -0.03, 0.01], [0, 0, 0.02]], np.float64)


@functools.lru_cache(None)
def image_set():
    """dict(descs, keypoints, depth [7, H, W], intr, Rcw, tcw, landmark (per image: the landmark of every key point, -1: none))"""
    synth = importlib.import_module("global-lvba_amd.synth")
    import torch
    rng = np.random.default_rng(20261019)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    W, H = synth.REF_IMAGE_WH
    n_land = N_SHARED + N_ONLY4
    X = np.zeros((n_land, 3))
    X[:, 0], X[:, 1] = rng.uniform(-1.8, 1.8, n_land), rng.uniform(-1.4, 1.4, n_land)
    X[:, 2] = mdc.PLANE_Z0 + mdc.PLANE_SLOPE * X[:, 0]
    tex = mc.sift_like(rng, n_land)
    Rcw = np.stack([mc._rot(*a) for a in ANGLES])
    tcw = -np.einsum("nij,nj->ni", Rcw, CENTRES)
    depth = np.stack([mdc.plane_depth(intr, Rcw[v], tcw[v], W, H) for v in range(len(COUNTS))])
    seen = {1: np.array([5]), 4: np.arange(n_land), 5: np.arange(N_SHARED)}       # landmark 5: images 1, 4 and 5
    descs, kps, landmark = [], [], []
    for v, n in enumerate(COUNTS):
        idx = rng.permutation(seen.get(v, np.zeros(0, np.int64)))
        n_dis = n - len(idx)
        uv = synth.project_distorted(torch.from_numpy(X[idx] @ Rcw[v].T + tcw[v]), intr).numpy().reshape(-1, 2) + rng.normal(0, 0.3, (len(idx), 2))
        assert ((uv > 2) & (uv < np.array([W - 3, H - 3]))).all()
        d = np.vstack([mc.noisy(rng, tex[idx], 6), mc.sift_like(rng, n_dis)]) if n else np.zeros((0, 128), np.uint8)
        k = np.vstack([uv, np.stack([rng.uniform(2, W - 3, n_dis), rng.uniform(2, H - 3, n_dis)], 1)]).astype(np.float32)
        descs.append(np.ascontiguousarray(d)); kps.append(k.reshape(-1, 2))
        landmark.append(np.concatenate([idx, np.full(n_dis, -1)]).astype(np.int64))
    return dict(descs=descs, keypoints=kps, depth=depth, intr=intr, Rcw=Rcw, tcw=tcw, landmark=landmark)


@functools.lru_cache(None)
def geometry():
    s = image_set()
    return mdo.DepthGeometry(s["keypoints"], s["intr"], s["Rcw"], s["tcw"], s["depth"])


def check_margins():
    s = image_set()
    return mdc.check_margins(s["descs"], PAIRS, MATCH_OPTION_SETS, geometry())


@functools.lru_cache(None)
def oracle_matches(guided):
    """(matches, scores, match_off) of PAIRS"""
    return mdo.match_pairs(image_set()["descs"], PAIRS, geometry(), guided=guided)


@functools.lru_cache(None)
def putative():
    """the unguided oracle matches of VERIFY_PAIRS, one array per pair: what the verifier and the track builder are given"""
    return [mdo.match_pair(image_set()["descs"], int(a), int(b), geometry(), guided=0)[0] for a, b in VERIFY_PAIRS]


@functools.lru_cache(None)
def undistorted():
    s = image_set()
    return [mo.undistort_all(s["intr"], k) for k in s["keypoints"]]


def _verify_args(p, kw):
    s = image_set()
    a, b = (int(x) for x in VERIFY_PAIRS[p])
    lo, hi = min(a, b), max(a, b)
    return (vo.points(undistorted(), a, b, putative()[p]), lo, hi, vo.relative_rotation(s["Rcw"][lo], s["Rcw"][hi])), dict(vo.DEFAULTS, intr=s["intr"], **kw)


@functools.lru_cache(None)
def oracle_verify(p, k):
    """verify_oracle.verify_pair of VERIFY_PAIRS[p] under VERIFY_OPTION_SETS[k]"""
    args, o = _verify_args(p, VERIFY_OPTION_SETS[k])
    return vo.verify_pair(*args, **o)


def hypothesis_margin():
    """the smallest relative margin of any inlier decision of any hypothesis the GPU test forms"""
    worst = np.inf
    for p in range(len(VERIFY_PAIRS)):
        for kw in VERIFY_OPTION_SETS:
            args, o = _verify_args(p, kw)
            if len(args[0]) >= vo.sample_size(o["method"]):
                worst = min(worst, vo.hypotheses(*args, with_margin=True, **o)[3])
    return worst
