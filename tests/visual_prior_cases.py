"""Problems and prior sets shared by tests/test_visual_priors_host.py and tests/test_gpu_visual_priors.py.  TEST INFRASTRUCTURE
ONLY: a helper module, not a test file."""
from __future__ import annotations

import importlib
import math

import numpy as np

DRIFT_BAR = 0.19          # twice the oracle's own ratio on drift_case (test_priors_pull_drifted_cameras_back_oracle)


def _L():
    return importlib.import_module("global-lvba_amd._lib")


def make_prior(kind, i, j, meas, sqrt_info, oi=None, oj=None):
    """An lvba_prior struct from raw arrays (kind 0 POSE / 1 POSITION / 2 RELATIVE; offsets of twelve zeros: the identity)."""
    p = _L().Prior()
    p.kind, p.i, p.j, p.reserved = int(kind), int(i), int(j), 0
    p.meas[:] = [float(v) for v in meas]
    p.offset_i[:] = [float(v) for v in (np.zeros(12) if oi is None else oi)]
    p.offset_j[:] = [float(v) for v in (np.zeros(12) if oj is None else oj)]
    p.sqrt_info[:] = [float(v) for v in np.asarray(sqrt_info, np.float64).reshape(36)]
    return p


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def quat_to_rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def world_poses(q, t):
    """T_world<-cam of every camera: (R [M,3,3], p [M,3])."""
    R = np.array([quat_to_rot(a).T for a in q])
    return R, -np.einsum("nij,nj->ni", R, np.asarray(t, np.float64))


def centres(q, t):
    return world_poses(q, t)[1]


def centre_rms(d, q, t):
    """RMS distance of the camera centres from the ground truth, camera 0 (constant, at its ground truth) left out."""
    return float(np.sqrt(np.mean(np.sum((centres(q, t) - centres(d["q_gt"], d["t_gt"]))[1:] ** 2, 1))))


def extrinsic(synth):
    """(Rci, tci) = T_cam<-imu of the synthetic rig, the rotation made orthonormal (the constants carry six digits)."""
    U, _, Vt = np.linalg.svd(np.asarray(synth._RCL, np.float64))
    Rci = U @ Vt
    return Rci, Rci @ np.asarray(synth._TLI, np.float64) + np.asarray(synth._PCL, np.float64)


def imu_poses(synth, q, t):
    """[M,12] T_world<-imu = T_world<-cam T_cam<-imu of the cameras (q, t)."""
    Rci, tci = extrinsic(synth)
    R, p = world_poses(q, t)
    return np.concatenate([np.einsum("nij,jk->nik", R, Rci).reshape(-1, 9), np.einsum("nij,j->ni", R, tci) + p], 1)


def mixed_priors(synth, d, seed=5, noise_rot=2e-3, noise_pos=0.02):
    """Priors of all three kinds on the problem d, measurements = ground truth + noise: a POSE prior on every third camera (with
    the extrinsic as offset, a full lower-triangular sqrt_info on one of them) and one on camera 0, POSITION priors with a lever
    arm on two cameras, RELATIVE priors between some consecutive cameras, one RELATIVE pair (1, M-1) far enough apart to share
    no landmark, and one RELATIVE pair with camera 0."""
    rng = np.random.default_rng(seed)
    M = d["q"].shape[0]
    Rci, tci = extrinsic(synth)
    O = np.r_[Rci.reshape(9), tci]
    Rw, pw = world_poses(d["q_gt"], d["t_gt"])

    def noisy(R, p):
        return np.r_[(R @ exp_so3(rng.normal(size=3) * noise_rot)).reshape(9), p + rng.normal(size=3) * noise_pos]

    def A(k, off):
        return (Rw[k] @ off[:9].reshape(3, 3), Rw[k] @ off[9:] + pw[k]) if off is not None else (Rw[k], pw[k])

    out = []
    diag = np.diag(1.0 / np.r_[[3e-3] * 3, [0.03] * 3])
    for n, k in enumerate([0] + list(range(2, M, 3))):
        Lm = diag if n != 1 else diag + np.tril(rng.normal(size=(6, 6)), -1) * 5.0
        out.append(make_prior(0, k, 0, noisy(*A(k, O)), Lm, O))
    for k in (1, M // 2):
        arm = np.r_[np.eye(3).reshape(9), rng.normal(size=3) * 0.3]
        z = A(k, arm)[1] + rng.normal(size=3) * noise_pos
        L3 = np.zeros((6, 6))
        L3[:3, :3] = np.diag([30.0, 30.0, 15.0]) + np.tril(rng.normal(size=(3, 3)), -1)
        out.append(make_prior(1, k, 0, np.r_[np.eye(3).reshape(9), z], L3, arm))
    pairs = [(k, k + 1) for k in range(1, M - 1, 2)] + [(M - 1, 1), (0, 3), (4, 0)]
    for n, (i, j) in enumerate(pairs):
        oi, oj = (O, O) if n % 2 == 0 else (None, None)
        (RA, pA), (RB, pB) = A(i, oi), A(j, oj)
        out.append(make_prior(2, i, j, noisy(RA.T @ RB, RA.T @ (pB - pA)), diag * 0.5, oi, oj))
    return out


def drift_case(pkg, synth, n_cams=8, n_tracks=60, seed=3, rot_deg=0.3, trans=0.06, sigma_rot=5e-4, sigma_pos=0.003):
    """Cameras started from a smooth drift that grows along the trajectory (camera k: a rotation of rot_deg k / (M - 1) about a
    fixed axis and a shift of trans k / (M - 1) along a fixed direction, both in the world frame), POSE priors at the true poses
    from pipeline.lidar_camera_priors.  Returns (d, oracle VisualProblem, priors)."""
    from oracle import visual_oracle as vo
    d = dict(synth.make_visual_problem(n_cams=n_cams, n_tracks=n_tracks, seed=seed))
    M = n_cams
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    direc = np.array([0.6, 0.7, -0.39]) / np.linalg.norm([0.6, 0.7, -0.39])
    Rw, pw = world_poses(d["q_gt"], d["t_gt"])
    q, t = d["q_gt"].copy(), d["t_gt"].copy()
    rot_to_quat = importlib.import_module("global-lvba_amd.pipeline").rot_to_quat_wxyz
    for k in range(1, M):
        f = k / (M - 1)
        R = exp_so3(axis * math.radians(rot_deg) * f) @ Rw[k]
        p = pw[k] + direc * trans * f
        q[k] = rot_to_quat(R.T)[0]
        t[k] = -R.T @ p
    d["q"], d["t"] = q, t
    Rci, tci = extrinsic(synth)
    priors = importlib.import_module("global-lvba_amd.pipeline").lidar_camera_priors(imu_poses(synth, d["q_gt"], d["t_gt"]), Rci, tci, sigma_rot, sigma_pos)
    p = vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    return d, p, priors
