"""CPU tests of the visual stage's camera pose priors: the torch model (tests/visual_prior_oracle.py) against central finite
differences through EigenQuaternionManifold::Plus, the device header csrc/visual_prior_device.h compiled for the host against
the model, and the behaviour the feature exists for (drifted cameras pulled back by priors) on the model alone."""
import math
import os
import subprocess

import numpy as np
import pytest

import visual_prior_oracle as vpo
from conftest import ROOT
from oracle.visual_oracle import eigen_quat_plus
from visual_prior_cases import drift_case, make_prior

KINDS = ["pose", "position", "relative"]
KIND_ID = {"pose": 0, "position": 1, "relative": 2}
CASES = [(k, off, reg) for k in KINDS for off in (False, True) for reg in ("ident", "three", "any")]


def _rand_rot(rng, angle=None):
    w = rng.normal(size=3)
    w *= (rng.uniform(0.1, 3.0) if angle is None else angle) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def _case(rng, kind, offsets, regime):
    """(prior on cameras 0 / 1, q [2, 4] un-normalised, t [2, 3]); the rotation residual near 0 ('ident'), at ~3 rad ('three') or
    anywhere"""
    q = rng.normal(size=(2, 4)) * rng.uniform(0.5, 2.0, size=(2, 1))         # |q| != 1: R normalises, Plus does not
    t = rng.normal(scale=5.0, size=(2, 3))
    o = [np.r_[_rand_rot(rng).reshape(9), rng.normal(size=3)] if offsets else np.zeros(12) for _ in range(2)]
    import torch
    A, B = [], None
    poses = []
    for k in range(2):
        R, p = vpo.world_pose(torch.tensor(q[k]), torch.tensor(t[k]))
        R, p = R.numpy(), p.numpy()
        Ro, po_ = (o[k][:9].reshape(3, 3), o[k][9:]) if offsets else (np.eye(3), np.zeros(3))
        poses.append((R @ Ro, R @ po_ + p))
    A, B = poses
    R_true = A[0] if kind != "relative" else A[0].T @ B[0]
    ang = {"ident": 1e-3, "three": 3.0, "any": None}[regime]
    Rm = R_true @ _rand_rot(rng, ang).T
    Lm = np.tril(rng.normal(size=(6, 6))) + 3.0 * np.eye(6)
    pr = make_prior(KIND_ID[kind], 0, 1 if kind == "relative" else 0, np.r_[Rm.reshape(9), rng.normal(size=3)], Lm, o[0], o[1])
    return pr, q, t


@pytest.mark.parametrize("kind,offsets,regime", CASES)
def test_oracle_jacobians_match_central_differences(kind, offsets, regime):
    rng = np.random.default_rng(1000 + CASES.index((kind, offsets, regime)))
    for _ in range(2):
        pr, q, t = _case(rng, kind, offsets, regime)
        e, Wi, Wj = vpo.prior_block(pr, q, t)
        if kind != "position":
            r = np.linalg.solve(np.array(list(pr.sqrt_info)).reshape(6, 6), e)
            if regime == "three":
                assert abs(np.linalg.norm(r[:3]) - 3.0) < 1e-9
            if regime == "ident":
                assert abs(np.linalg.norm(r[:3]) - 1e-3) < 1e-9
        else:
            assert not e[3:].any() and not Wi[3:].any()
        h = 1e-6
        for cam, W in ((0, Wi), (1, Wj)):
            num = np.zeros((6, 6))
            for c in range(6):
                out = []
                for sgn in (1.0, -1.0):
                    q2, t2 = q.copy(), t.copy()
                    d = np.zeros(6)
                    d[c] = sgn * h
                    q2[cam] = eigen_quat_plus(q[cam], d[:3])
                    t2[cam] = t[cam] + d[3:]
                    out.append(vpo.prior_block(pr, q2, t2, False)[0])
                num[:, c] = (out[0] - out[1]) / (2 * h)
            if cam == 1 and kind != "relative":
                assert not W.any()
            assert np.abs(num - W).max() <= 1e-6 * max(1.0, np.abs(W).max()), (kind, cam, num - W)


def test_device_header_agrees_with_the_oracle(tmp_path):
    """csrc/visual_prior_device.h (host build) vs the torch model: whitened residuals, both whitened Jacobian blocks and the cost
    to 1e-11 of each quantity's scale."""
    exe = str(tmp_path / "visual_prior_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "visual_prior_check.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    ident = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    lines, cases = [], []
    for kind, off, reg in CASES * 3:
        pr, q, t = _case(rng, kind, off, reg)
        cases.append((pr, q, t))
        oi, oj = (np.array(list(o)) for o in (pr.offset_i, pr.offset_j))
        vals = np.r_[q[0], t[0], q[1], t[1], oi if oi.any() else ident, oj if oj.any() else ident, np.array(list(pr.meas)),
                     np.array(list(pr.sqrt_info))]
        lines.append(f"{pr.kind} " + " ".join(float(v).hex() for v in vals))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    worst = 0.0
    for (pr, q, t), ln in zip(cases, out):
        v = np.array([float.fromhex(x) for x in ln.split()])
        assert v.size == 6 + 36 + 36 + 1
        e, Wi, Wj = vpo.prior_block(pr, q, t)
        for got, ref in ((v[:6], e), (v[6:42], Wi.reshape(-1)), (v[42:78], Wj.reshape(-1)), (v[78:], [0.5 * e @ e])):
            ref = np.asarray(ref)
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.any() else np.abs(got).max()
            worst = max(worst, err)
            assert err <= 1e-11, (pr.kind, err)
    print("worst relative difference", worst)


def test_no_priors_is_the_parent_bit_for_bit(synth):
    from oracle import visual_oracle as vo
    from robust_visual_oracle import RobustVisualOracle
    d = synth.make_visual_problem(n_cams=4, n_tracks=12, seed=3)
    p = vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    for losses in ((None, None), (("huber", 1.0), ("huber", 0.1))):
        a, b = vpo.VisualPriorOracle(p, [], *losses), RobustVisualOracle(p, *losses)
        q, t, X = a.state()
        for u, v in zip(a.residuals_and_jacobian(q, t, X), b.residuals_and_jacobian(q, t, X)):
            assert np.array_equal(u, v)
        assert a.cost(q, t, X) == b.cost(q, t, X)
        Sa, ra, ca = a.linearization(q, t, X, 3.0)
        Sb, rb, cb = b.linearization(q, t, X, 3.0)
        assert np.array_equal(Sa, Sb) and np.array_equal(ra, rb) and ca == cb


def test_priors_pull_drifted_cameras_back_oracle(pkg, synth):
    """The behavioural case of tests/test_gpu_visual_priors.py on the model alone (visual_prior_cases.drift_case: 8 cameras x 60
    landmarks, seed 3, a smooth drift growing to 6 cm / 0.3 deg along the trajectory, POSE priors at the true poses from
    pipeline.lidar_camera_priors with sigma 0.0005 rad / 0.003 m).  RMS camera-centre error: 0.03833 m at the start, 0.02013 m
    after the refinement without priors, 0.001903 m with them: ratio 0.0945.  The bar is twice that, 0.19
    (visual_prior_cases.DRIFT_BAR)."""
    from visual_prior_cases import DRIFT_BAR, centre_rms
    d, p, priors = drift_case(pkg, synth)
    (q0, t0, _), _, _ = vpo.VisualPriorOracle(p).solve()
    (q1, t1, _), _, _ = vpo.VisualPriorOracle(p, priors).solve()
    e0, e1 = centre_rms(d, q0, t0), centre_rms(d, q1, t1)
    print("camera-centre RMS without / with priors:", e0, e1, "ratio", e1 / e0)
    assert e1 < DRIFT_BAR * e0
