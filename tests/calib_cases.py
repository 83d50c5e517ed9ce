"""Seeded cases of the extrinsic refinement (tests/calib_oracle.py).  A case is a trajectory of body poses, a true
extrinsic, a planted wrong one, and records made backwards from the target side so that they are exact: a pixel of image a that
fp32 holds exactly, undistorted by the oracle, pushed out to a depth, and carried into the source camera b through the TRUE cameras.
At the true extrinsic a noise-free record's residual is rounding (1e-12 px).
  general   the body rotates about three axes: every direction of the extrinsic is observable.
  screw     the body turns about its z axis and moves along it only: the rotation about that axis and the translation along it are
            not observable (two held directions).
  planar    a ground vehicle: it turns about z and moves ACROSS it.  The motion across the axis ties the rotation about it down
            through the LiDAR's metric scale; only the translation along the axis stays unobservable (one held direction)."""
import functools
import os
import re

import numpy as np

import calib_oracle as co

INTR = np.array([600.0, 590.0, 320.0, 256.0, -0.05, 0.01, 0.001, -0.0005])
WIDTH, HEIGHT = 640, 512
PLANT_ROT_DEG, PLANT_TRANS = 3.0, 0.10
# T_cam<-imu of a camera that looks along the body's x axis (z forward, x right, y down), turned a little, 12 cm off the origin
R_TRUE = (co.rodrigues([0.02, -0.03, 0.015]) @ np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])).reshape(9)
T_TRUE = np.array([0.05, -0.10, 0.03])

# What the order of summation alone changes in the refined extrinsic of noisy(): the largest difference, over the nine entries of R
# and the three of t, between the oracle's run with every sum taken in index order and its run with every sum taken in reversed
# order, measured on the CPU (tests/test_calib_host.py::test_order_of_summation_on_the_noisy_case prints and re-measures it).
# The device's sums are a third order (a tree); its extrinsic is held to 16 times this against the oracle's index-order run.
NOISY_ORDER_D = 8.9e-16
NOISY_TOL = 16 * NOISY_ORDER_D


def header_constants():
    """the integer constants of csrc/calib_device.h by name (CAL_NS, CAL_BLOCK, CAL_RUN, CAL_MAX_BLOCKS, ...)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "global-lvba_amd", "csrc", "calib_device.h")
    out = {}
    for decl in re.findall(r"constexpr int ([^;]*);", open(path).read()):
        for name, value in re.findall(r"(CAL_\w+) = (\d+)", decl):
            out[name] = int(value)
    return out


def camera_from_imu(poses, R, t):
    """Rcw = Rci Rwi^T, tcw = -Rcw Pwi + tci (pipeline.camera_from_imu)"""
    T = np.asarray(poses, np.float64).reshape(-1, 12)
    Rwi, P = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    Rcw = np.einsum("ij,nkj->nik", np.asarray(R).reshape(3, 3), Rwi)
    return Rcw, -np.einsum("nij,nj->ni", Rcw, P) + np.asarray(t).reshape(3)


def trajectory(kind, M, rng):
    poses = np.zeros((M, 12))
    R, P = np.eye(3), np.zeros(3)
    for k in range(M):
        if k:
            if kind == "general":
                R = R @ co.rodrigues(rng.uniform(-0.15, 0.15, 3))
                P = P + rng.uniform(-0.3, 0.3, 3)
            else:
                R = R @ co.rodrigues([0.0, 0.0, rng.uniform(0.08, 0.2)])
                P = P + (np.array([0.0, 0.0, rng.uniform(0.05, 0.2)]) if kind == "screw" else
                         R @ np.array([rng.uniform(0.2, 0.4), rng.uniform(-0.05, 0.05), 0.0]))
        poses[k, :9], poses[k, 9:] = R.reshape(9), P
    return poses


def directed_pairs(M, span):
    """both directions of every pair (a, b), a < b <= a + span: (a, b) then (b, a)"""
    out = []
    for a in range(M):
        for b in range(a + 1, min(M, a + span + 1)):
            out += [(a, b), (b, a)]
    return np.array(out, np.int32).reshape(-1, 2)


def make(kind, M=10, per_pair=400, span=2, seed=0, noise_px=0.0, outliers=0.0):
    rng = np.random.default_rng(seed)
    poses = trajectory(kind, M, rng)
    Rcw, tcw = camera_from_imu(poses, R_TRUE, T_TRUE)
    pairs = directed_pairs(M, span)
    P = len(pairs)
    n = P * per_pair
    pair = np.repeat(np.arange(P, dtype=np.int32), per_pair)
    a, b = pairs[pair, 0], pairs[pair, 1]
    uv = (np.round(rng.uniform([20, 20], [WIDTH - 20, HEIGHT - 20], (n, 2)) * 16) / 16).astype(np.float32)   # exact in fp32
    xy = co.undistort(INTR, uv)
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
    d = rng.normal(size=3)
    e = rng.normal(size=3)
    om = d / np.linalg.norm(d) * np.radians(PLANT_ROT_DEG)
    R0 = (co.rodrigues(om) @ R_TRUE.reshape(3, 3)).reshape(9)
    t0 = T_TRUE + e / np.linalg.norm(e) * PLANT_TRANS
    return dict(name=kind, poses=poses, intr=INTR, img_a=np.ascontiguousarray(pairs[:, 0]), img_b=np.ascontiguousarray(pairs[:, 1]),
                pair=pair, uv=np.ascontiguousarray(uv), Xb=np.ascontiguousarray(Xb), R_true=R_TRUE, t_true=T_TRUE, R0=R0, t0=t0,
                outlier=planted)


@functools.lru_cache(None)
def general():
    return make("general", seed=11)


@functools.lru_cache(None)
def screw():
    return make("screw", seed=12)


@functools.lru_cache(None)
def planar():
    return make("planar", seed=13)


@functools.lru_cache(None)
def noisy():
    """the general trajectory with 0.5 px of noise and 20 % gross outliers (20 .. 80 px off)"""
    return make("general", seed=14, noise_px=0.5, outliers=0.2)


@functools.lru_cache(None)
def wide(n):
    """at least n records over few pairs, for the edges of the kernel's partition: tests take a prefix"""
    P = 6
    return make("general", M=4, per_pair=(n + P - 1) // P, span=1, seed=15)


# ---- a small LiDAR-camera sequence for pipeline.calibrate_extrinsic: a box room scanned and photographed from its middle by a body
# that turns about three axes (up to 17 degrees each) and moves little (half a metre): the motion of a hand-held scanner
ROOM = np.array([14.0, 10.0, 4.0])
ROOM_RCI = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # the camera looks along the body's y axis
ROOM_TCI = np.array([0.02, 0.05, -0.03])
ROOM_INTR = np.array([300.0, 298.0, 240.0, 180.0, -0.076160, 0.123001, -0.00113, 0.000251])
ROOM_W, ROOM_H = 480, 360
ROOM_PLANT = np.r_[np.radians(2.0) * np.array([0.6, -0.48, 0.64]), 0.06, -0.08, 0.04]   # 2 degrees, 10.8 cm


def _room_hit(c, ray):
    """where the rays from c (inside the room) leave the box"""
    with np.errstate(all="ignore"):
        tt = np.where(ray > 0, (ROOM / 2 - c) / ray, (-ROOM / 2 - c) / ray)
    return c + tt.min(axis=1)[:, None] * ray


@functools.lru_cache(None)
def room_sequence(M=8, pts=80000, n_land=500, seed=5):
    """dict(clouds [M] float32 body-frame scans, poses [M, 12] = T_world<-imu of scans and images alike, times, kps, pairs, matches):
    landmarks on the walls in front, seen with 0.4 px of noise from the true cameras camera_from_imu(poses, ROOM_RCI, ROOM_TCI);
    every pair of images is matched through the landmarks' identities"""
    from oracle import track_oracle as to
    rng = np.random.default_rng(seed)
    poses = np.zeros((M, 12))
    clouds = []
    for k in range(M):
        R = co.rodrigues(rng.uniform(-0.3, 0.3, 3))
        P = rng.uniform(-0.5, 0.5, 3)
        poses[k, :9], poses[k, 9:] = R.reshape(9), P
        # a scanner that looks where the camera looks (the body's y axis): the depth images are point splats read bilinearly, and a
        # keypoint has a depth only where all four pixels around it hold a return
        d = (rng.normal(size=(pts, 3)) * [0.9, 0.0, 0.75] + [0.0, 1.0, 0.0]) @ R.T
        w = _room_hit(P, d / np.linalg.norm(d, axis=1, keepdims=True)) + rng.normal(0.0, 0.005, (pts, 3))
        clouds.append(np.ascontiguousarray(((w - P) @ R).astype(np.float32)))
    Rcw, tcw = camera_from_imu(poses, ROOM_RCI, ROOM_TCI)
    d = rng.normal(size=(n_land, 3))
    d[:, 1] = np.abs(d[:, 1]) + 1.0
    X = _room_hit(np.zeros(3), d / np.linalg.norm(d, axis=1, keepdims=True))
    kps, ids = [], []
    for m in range(M):
        k, seen = [], []
        for li, x in enumerate(X):
            p = to.project(ROOM_INTR, Rcw[m], tcw[m], x)
            if p is not None and 3 < p[0] < ROOM_W - 4 and 3 < p[1] < ROOM_H - 4:
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
    return dict(clouds=clouds, poses=poses, times=50.0 + 0.1 * np.arange(M), kps=kps, pairs=pairs, matches=matches)


def held_span(kind, R, t):
    """[k, 6]: an orthonormal basis of the unobservable left perturbations (om, up) at (R, t), from the theory: a perturbation
    X Z X^-1 with Z commuting with every body motion.  z the body's axis in the camera frame: screw -> (z, t x z) and (0, z);
    planar -> (0, z); general -> none."""
    z = np.asarray(R).reshape(3, 3) @ np.array([0.0, 0, 1])
    rows = {"general": [], "planar": [np.r_[0, 0, 0, z]], "screw": [np.r_[z, np.cross(np.asarray(t).reshape(3), z)], np.r_[0, 0, 0, z]]}[kind]
    if not rows:
        return np.zeros((0, 6))
    q, _ = np.linalg.qr(np.array(rows).T)
    return q.T


def principal_angles(U, V):
    """the principal angles (radians) between the row spaces of U and V (orthonormal rows)"""
    s = np.linalg.svd(np.asarray(U) @ np.asarray(V).T, compute_uv=False)
    # sin from the residual, which keeps small angles: |V - (V U^T) U| per direction
    res = np.asarray(V) - (np.asarray(V) @ np.asarray(U).T) @ np.asarray(U)
    return np.arcsin(np.clip(np.linalg.svd(res, compute_uv=False), 0.0, 1.0)) if len(s) else np.zeros(0)


def args(case, n=None):
    """the positional arguments of calib.refine_extrinsic / calib.linearize up to the extrinsic, over the first n records"""
    n = len(case["pair"]) if n is None else n
    records = dict(pair=case["pair"][:n], uv=case["uv"][:n], Xb=case["Xb"][:n])
    return records, (case["img_a"], case["img_b"]), case["poses"], case["intr"]
