"""Seeded cases of the extrinsic refinement with a time offset (tests/calib_td_oracle.py; DESIGN.md §10o "time offset").  None is
committed.  The GIVEN body poses come from calib_cases.trajectory; every image has a seeded twist; the TRUE body poses are the given
ones shifted by td_true under the rule's own model (calib_td_oracle.shift_poses).  Records are made backwards from fp32-exact
pixels through the true cameras, as calib_cases.make makes them: at the true extrinsic and the true offset a noise-free record's
residual is rounding.
  general   twists in every direction, up to 0.5 rad/s and 1 m/s: seven observable directions.
  planar    a ground vehicle: it turns about z and moves across it, and so do its twists: the translation along z is held.
  screw     poses exp(k dt xi) of ONE body-frame twist xi whose translation is along its rotation axis, and that twist at every
            image: A(td) does not depend on td, so the td axis is held beside the screw's two directions.
  zero      the general trajectory with zero twists: the 6-parameter problem."""
import functools
import os
import re

import numpy as np

import calib_cases as cc
import calib_oracle as co
import calib_td_oracle as cto

MAX_OMEGA, MAX_V = 0.5, 1.0

# What the order of summation alone changes in the refined (R, t, td) of noisy(): the largest difference, over the nine entries of
# R, the three of t and td, between the oracle's run with every sum in index order and its run with every sum in reversed order,
# measured on the CPU (tests/test_calib_td_host.py::test_order_of_summation_on_the_noisy_case prints and re-measures it).  The
# device's sums are a third order (a tree); its result is held to 16 times this against the oracle's index-order run.
NOISY_ORDER_D = 4.5e-16
NOISY_TOL = 16 * NOISY_ORDER_D


def header_constants():
    """the integer constants of csrc/calib_device.h and csrc/calib_td_device.h by name (CAL_BLOCK, CAL_TD_NS, ...)"""
    out = cc.header_constants()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "global-lvba_amd", "csrc", "calib_td_device.h")
    for decl in re.findall(r"constexpr int ([^;]*);", open(path).read()):
        for name, value in re.findall(r"(CAL_\w+) = (\d+)", decl):
            out[name] = int(value)
    return out


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def seeded_twists(kind, poses, rng):
    """[M, 6]: om (body frame) of 0.25 .. 0.5 rad/s and v (world frame) of 0.5 .. 1 m/s per image, in the plane's sense for planar"""
    M = len(poses)
    om = unit(rng, M) * rng.uniform(0.5 * MAX_OMEGA, MAX_OMEGA, (M, 1))
    v = unit(rng, M) * rng.uniform(0.5 * MAX_V, MAX_V, (M, 1))
    if kind == "planar":
        om = np.stack([np.zeros(M), np.zeros(M), rng.uniform(0.5 * MAX_OMEGA, MAX_OMEGA, M) * rng.choice([-1.0, 1.0], M)], 1)
        ang = rng.uniform(0, 2 * np.pi, M)
        v = np.stack([np.cos(ang), np.sin(ang), np.zeros(M)], 1) * rng.uniform(0.5 * MAX_V, MAX_V, (M, 1))
    return np.concatenate([om, v], 1)


def screw_motion(M, rng, dt=0.4):
    """(poses [M, 12], twists [M, 6]) of one body-frame twist (om, pitch om) about a seeded axis: T_k = exp(k dt xi)"""
    axis = unit(rng, 1)[0]
    om, u = 0.45 * axis, 0.6 * axis
    poses, twists = np.zeros((M, 12)), np.zeros((M, 6))
    for k in range(M):
        R = co.rodrigues(k * dt * om)
        poses[k, :9], poses[k, 9:] = R.reshape(9), k * dt * u               # u is along the axis: V(th) u = u
        twists[k, :3], twists[k, 3:] = om, R @ u                             # (R u = u: the world-frame velocity)
    return poses, twists, axis


def make(kind, td_true=0.02, M=10, per_pair=400, span=2, seed=0, noise_px=0.0, outliers=0.0):
    rng = np.random.default_rng(seed)
    axis = None
    if kind == "screw":
        poses, twists, axis = screw_motion(M, rng)
    else:
        poses = cc.trajectory("general" if kind == "zero" else kind, M, rng)
        twists = np.zeros((M, 6)) if kind == "zero" else seeded_twists(kind, poses, rng)
    true_poses = cto.shift_poses(poses, twists, td_true)
    Rcw, tcw = cc.camera_from_imu(true_poses, cc.R_TRUE, cc.T_TRUE)
    pairs = cc.directed_pairs(M, span)
    P = len(pairs)
    n = P * per_pair
    pair = np.repeat(np.arange(P, dtype=np.int32), per_pair)
    a, b = pairs[pair, 0], pairs[pair, 1]
    uv = (np.round(rng.uniform([20, 20], [cc.WIDTH - 20, cc.HEIGHT - 20], (n, 2)) * 16) / 16).astype(np.float32)   # exact in fp32
    xy = co.undistort(cc.INTR, uv)
    z = rng.uniform(3.0, 12.0, n)
    Xa = np.stack([xy[:, 0] * z, xy[:, 1] * z, z], 1)
    world = np.einsum("nji,nj->ni", Rcw[a], Xa - tcw[a])
    Xb = np.einsum("nij,nj->ni", Rcw[b], world) + tcw[b]
    assert Xb[:, 2].min() > 0.5
    planted = np.zeros(n, bool)
    if noise_px:
        uv = (uv.astype(np.float64) + rng.normal(0.0, noise_px, (n, 2))).astype(np.float32)
    if outliers:
        planted = rng.random(n) < outliers
        ang = rng.uniform(0, 2 * np.pi, n)
        off = rng.uniform(20.0, 80.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        uv = np.where(planted[:, None], (uv.astype(np.float64) + off).astype(np.float32), uv)
    d, e = unit(rng, 1)[0], unit(rng, 1)[0]
    R0 = (co.rodrigues(d * np.radians(cc.PLANT_ROT_DEG)) @ cc.R_TRUE.reshape(3, 3)).reshape(9)
    t0 = cc.T_TRUE + e * cc.PLANT_TRANS
    return dict(name=kind, poses=poses, twists=twists, td_true=float(td_true), true_poses=true_poses, intr=cc.INTR,
                img_a=np.ascontiguousarray(pairs[:, 0]), img_b=np.ascontiguousarray(pairs[:, 1]), pair=pair, uv=np.ascontiguousarray(uv),
                Xb=np.ascontiguousarray(Xb), R_true=cc.R_TRUE, t_true=cc.T_TRUE, R0=R0, t0=t0, outlier=planted, axis=axis)


@functools.lru_cache(None)
def general(td_true=0.02):
    return make("general", td_true, seed=21)


@functools.lru_cache(None)
def planar():
    return make("planar", 0.02, seed=23)


@functools.lru_cache(None)
def screw():
    return make("screw", 0.0, seed=22)


@functools.lru_cache(None)
def zero():
    return make("zero", 0.0, seed=24)


@functools.lru_cache(None)
def noisy():
    """the general trajectory with 0.5 px of noise and 20 % gross outliers (20 .. 80 px off)"""
    return make("general", 0.02, seed=25, noise_px=0.5, outliers=0.2)


@functools.lru_cache(None)
def wide(n):
    """at least n records over few pairs, for the edges of the kernel's partition: tests take a prefix"""
    P = 6
    return make("general", 0.02, M=4, per_pair=(n + P - 1) // P, span=1, seed=26)


def screw_held_span(case, R, t):
    """[3, 7]: an orthonormal basis of what the screw case leaves unobservable at (R, t): with z the screw's axis in the camera
    frame, the turn about it (z, t x z, 0), the shift along it (0, z, 0), and the td axis"""
    z = np.asarray(R).reshape(3, 3) @ case["axis"]
    rows = [np.r_[z, np.cross(np.asarray(t).reshape(3), z), 0.0], np.r_[0, 0, 0, z, 0.0], np.r_[np.zeros(6), 1.0]]
    q, _ = np.linalg.qr(np.array(rows).T)
    return q.T


def args(case, n=None):
    """the positional arguments of calib.refine_extrinsic_td / calib.linearize_td up to the extrinsic, over the first n records"""
    n = len(case["pair"]) if n is None else n
    records = dict(pair=case["pair"][:n], uv=case["uv"][:n], Xb=case["Xb"][:n])
    return records, (case["img_a"], case["img_b"]), case["poses"], case["twists"], case["intr"]


# ---- calib_cases.room_sequence with a time offset: the scans are taken at the given poses, the images at the poses shifted by
# ROOM_TD under seeded twists
ROOM_TD = 0.03


@functools.lru_cache(None)
def room_sequence(M=8, pts=80000, n_land=500, seed=5):
    """calib_cases.room_sequence's dict plus twists [M, 6] and td_true: the landmarks are seen from the cameras
    camera_from_imu(shift_poses(poses, twists, ROOM_TD), ROOM_RCI, ROOM_TCI)"""
    from oracle import track_oracle as to
    rng = np.random.default_rng(seed)
    poses = np.zeros((M, 12))
    clouds = []
    for k in range(M):
        R = co.rodrigues(rng.uniform(-0.3, 0.3, 3))
        P = rng.uniform(-0.5, 0.5, 3)
        poses[k, :9], poses[k, 9:] = R.reshape(9), P
        d = (rng.normal(size=(pts, 3)) * [0.9, 0.0, 0.75] + [0.0, 1.0, 0.0]) @ R.T
        w = cc._room_hit(P, d / np.linalg.norm(d, axis=1, keepdims=True)) + rng.normal(0.0, 0.005, (pts, 3))
        clouds.append(np.ascontiguousarray(((w - P) @ R).astype(np.float32)))
    twists = seeded_twists("general", poses, rng)
    Rcw, tcw = cc.camera_from_imu(cto.shift_poses(poses, twists, ROOM_TD), cc.ROOM_RCI, cc.ROOM_TCI)
    d = rng.normal(size=(n_land, 3))
    d[:, 1] = np.abs(d[:, 1]) + 1.0
    X = cc._room_hit(np.zeros(3), d / np.linalg.norm(d, axis=1, keepdims=True))
    kps, ids = [], []
    for m in range(M):
        k, seen = [], []
        for li, x in enumerate(X):
            p = to.project(cc.ROOM_INTR, Rcw[m], tcw[m], x)
            if p is not None and 3 < p[0] < cc.ROOM_W - 4 and 3 < p[1] < cc.ROOM_H - 4:
                k.append(np.float32(p) + np.float32(0.4 * rng.standard_normal(2)))
                seen.append(li)
        kps.append(np.array(k, np.float32).reshape(-1, 2))
        ids.append(seen)
    pairs, matches = [], []
    for i in range(M):
        for j in range(i + 1, M):
            pos = {li: kj for kj, li in enumerate(ids[j])}
            m = [(ki, pos[li]) for ki, li in enumerate(ids[i]) if li in pos]
            if m:
                pairs.append((i, j))
                matches.append(np.array(m, np.int64))
    return dict(clouds=clouds, poses=poses, twists=twists, td_true=ROOM_TD, times=50.0 + 0.1 * np.arange(M), kps=kps, pairs=pairs,
                matches=matches)
