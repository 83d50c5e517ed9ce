"""The shared place-recognition fixtures of tests/test_place_host.py and tests/test_gpu_place.py, computed once per process.

Two-lap fixture: lap A is loop_cases' scan set (12 frames, one closed loop in a room of 8 x 6 x 3 m); lap B is the even frames
of the same generator call with 24 frames -- the same scene, the same twelve positions and headings, fresh rays and fresh
roll/pitch noise.  Frame 12 + k is lap B's frame k re-expressed in a body turned by DELTA[k] = (k mod 5 + 1) sector angles plus
0.4 degrees about its own z.  The "drifted" poses leave lap A at the truth and move lap B rigidly by DRIFT_X along x and
DRIFT_YAW about z, farther than any pose radius finds.  The study behind the values is DESIGN.md §10e.

Synthetic descriptor sets: the analogue of loop_cases.laps for the search alone -- 130 frames from 40 random sparse images with
exact duplicates, rolled copies and an all-zero descriptor.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np

from oracle import voxel_oracle as vo
import loop_cases as lc
import loop_oracle as lo
import place_oracle as po
import register_oracle as ro

N_LAP = 12
PLACE = dict(n_rings=20, n_sectors=60, max_range=8.0, min_range=0.3, z_offset=2.5, submap_size=3, min_gap=10, n_key_candidates=4,
             max_per_frame=1)
SECTOR = 2.0 * po.PI / PLACE["n_sectors"]
EXTRA = np.radians(0.4)
DRIFT_X, DRIFT_YAW = 9.0, np.radians(10.0)
POSE_RADIUS = 2.5
LEVELLED = False
# the registration of a descriptor candidate: the start is off by the yaw quantisation (<= 3 degrees) and the roll/pitch noise
REG = dict(lc.OPTS, max_distance=0.25, loss=("cauchy", 0.05))
ACCEPT = dict(min_inlier_frac=0.3, max_rmse=0.05)


def planted(k):
    """Sectors by which lap B's frame k is turned."""
    return k % 5 + 1


@functools.lru_cache(maxsize=None)
def _laps():
    synth = importlib.import_module("global-lvba_amd.synth")
    a = lc.scans()
    b = synth.make_scans(2 * N_LAP, 3000, room=(8, 6, 3), origin=(2.5, -1.5, 0.2), n_panels=6, seed=5, noise=lc.NOISE, clutter_frac=0.05)
    clouds, poses = [c[:, :3].copy() for c in a["clouds"]], [p.copy() for p in a["poses_gt"]]
    for k in range(N_LAP):
        d = planted(k) * SECTOR + EXTRA
        T = b["poses_gt"][2 * k]
        cloud = b["clouds"][2 * k][:, :3].astype(np.float64) @ po.rz(-d).T          # Rz(-d) p
        clouds.append(cloud.astype(np.float32))
        poses.append(np.r_[(T[:9].reshape(3, 3) @ po.rz(d)).reshape(9), T[9:]])
    poses = np.stack(poses)
    if LEVELLED:
        for f in range(len(clouds)):
            R = poses[f, :9].reshape(3, 3)
            yaw = np.arctan2(R[1, 0], R[0, 0])
            lev = po.rz(-yaw) @ R                                               # the roll/pitch part: p_levelled = lev p
            clouds[f] = (clouds[f].astype(np.float64) @ lev.T).astype(np.float32)
            poses[f, :9] = po.rz(yaw).reshape(9)
    return dict(clouds=clouds, poses_gt=poses, lap_b_positions=b["poses_gt"][::2, 9:].copy())


def clouds():
    return _laps()["clouds"]


def truth():
    return _laps()["poses_gt"].copy()


def lap_b_positions():
    return _laps()["lap_b_positions"].copy()


@functools.lru_cache(maxsize=None)
def _drifted():
    P = truth()
    G, t = po.rz(DRIFT_YAW), np.array([DRIFT_X, 0.0, 0.0])
    for f in range(N_LAP, 2 * N_LAP):
        P[f] = np.r_[(G @ P[f, :9].reshape(3, 3)).reshape(9), G @ P[f, 9:] + t]
    return P


def drifted():
    return _drifted().copy()


@functools.lru_cache(maxsize=None)
def descriptors():
    """(desc [24, Nr, Ns], ring_key [24, Nr]) of the two laps by the oracle."""
    got = [po.descriptor(c, **PLACE) for c in clouds()]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def candidates():
    """(list, decision margin) of the two-lap fixture by the oracle."""
    return po.candidates(descriptors()[0], with_margin=True, **PLACE)


def pose_candidates(poses):
    return lo.candidates(poses, submap_size=PLACE["submap_size"], min_gap=PLACE["min_gap"], max_per_frame=PLACE["max_per_frame"],
                         query_stride=1, radius=POSE_RADIUS)


@functools.lru_cache(maxsize=None)
def oracle_submap(w):
    """The oracle's plane map of submap w at the drifted poses."""
    P, S = _drifted(), PLACE["submap_size"]
    fr = range(w * S, min((w + 1) * S, len(P)))
    surf, _ = vo.build([clouds()[f] for f in fr], P[fr.start:fr.stop], lc.VS, lc.RATIO)
    return surf


@functools.lru_cache(maxsize=None)
def oracle_register(query, w, ref, shift):
    """(start, registration, (accepted, reason)) of a descriptor candidate by the oracle, at the drifted poses."""
    start = po.start_pose(_drifted()[ref], po.yaw_of(shift, PLACE["n_sectors"]))
    reg = ro.register(oracle_submap(w), lc.VS, start, clouds()[query], **REG)
    rot, trans = lo.correction(start, reg["pose"])
    return start, reg, lo.accept(reg["status"], reg["inliers"], reg["points"], reg["rmse"], rot, trans, **ACCEPT)


# ---- synthetic descriptor sets ----------------------------------------------------------------------------------------------------
def synthetic(nr, ns, n=130, n_base=40, seed=3):
    """([n, nr, ns] float32, roll [n]): n_base random sparse images with values in [0, 4) and some empty columns; the next n_base
    frames are the images rolled by roll[f] sectors with a seventh of their cells halved (the same ring keys, hence exact ties in
    key distance, but a distance clearly above 0 -- two copies that differ in rounding alone would decide by the last bit); then
    exact duplicates of the images (exact ties in distance, resolved by f and by w); then rolled copies again.  Frame
    min(77, n - 1) is an all-zero descriptor."""
    rng = np.random.default_rng(seed + 1000 * nr + ns)
    base = (rng.random((n_base, nr, ns)) * 4.0).astype(np.float32)
    base[rng.random((n_base, nr, ns)) < 0.5] = 0.0
    for b in base:
        b[:, rng.random(ns) < 0.15] = 0.0
    out, roll = np.zeros((n, nr, ns), np.float32), np.zeros(n, np.int64)
    for f in range(n):
        img = base[f % n_base].copy()
        if (f // n_base) % 2 == 1:
            roll[f] = (7 * f + 3) % ns
            img[rng.random((nr, ns)) < 1.0 / 7.0] *= np.float32(0.5)
        out[f] = np.roll(img, roll[f], axis=1)
    out[min(77, n - 1)] = 0.0
    return out, roll


@functools.lru_cache(maxsize=None)
def syn(nr, ns):
    n = 130 if (nr, ns) != (32, 128) else 24
    return synthetic(nr, ns, n=n, n_base=40 if n == 130 else 8)


def search_cases():
    """(name, desc, options, capacity): every descriptor search the tests run."""
    base = dict(min_range=0.5, max_range=80.0, z_offset=2.0)
    g = lambda nr, ns, **kw: dict(base, n_rings=nr, n_sectors=ns, **kw)
    return [
        ("defaults-like", syn(20, 60)[0], g(20, 60, submap_size=5, min_gap=20, n_key_candidates=6, max_per_frame=2, query_stride=1, max_distance=0.4), None),
        ("cut to 1", syn(20, 60)[0], g(20, 60, submap_size=5, min_gap=20, n_key_candidates=8, max_per_frame=1, query_stride=1, max_distance=0.4), None),
        ("max_distance 1", syn(20, 60)[0], g(20, 60, submap_size=4, min_gap=10, n_key_candidates=5, max_per_frame=3, query_stride=1, max_distance=1.0), None),
        ("query_stride 2", syn(20, 60)[0], g(20, 60, submap_size=4, min_gap=10, n_key_candidates=5, max_per_frame=3, query_stride=2, max_distance=0.4), None),
        ("capacity", syn(20, 60)[0], g(20, 60, submap_size=5, min_gap=20, n_key_candidates=6, max_per_frame=2, query_stride=1, max_distance=0.4), 7),
        ("K = 32, one submap per frame", syn(7, 13)[0], g(7, 13, submap_size=1, min_gap=0, n_key_candidates=32, max_per_frame=32, query_stride=3, max_distance=0.5), None),
        ("7 x 13", syn(7, 13)[0], g(7, 13, submap_size=6, min_gap=15, n_key_candidates=5, max_per_frame=2, query_stride=1, max_distance=0.3), None),
        ("90 sectors", syn(10, 90)[0], g(10, 90, submap_size=5, min_gap=20, n_key_candidates=4, max_per_frame=2, query_stride=1, max_distance=0.4), None),
        ("32 x 128", syn(32, 128)[0], g(32, 128, submap_size=2, min_gap=4, n_key_candidates=3, max_per_frame=2, query_stride=1, max_distance=0.4), None),
        ("n < submap_size", syn(7, 13)[0][:3], g(7, 13, submap_size=5, min_gap=0, n_key_candidates=4, max_per_frame=2, query_stride=1, max_distance=1.0), None),
    ]


@functools.lru_cache(maxsize=None)
def search_oracle(k):
    name, desc, o, cap = search_cases()[k]
    return po.candidates(desc, with_margin=True, **o)
