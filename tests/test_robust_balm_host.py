"""CPU tests of the LiDAR stage's robust losses (lvba_balm_set_loss): the reference model tests/robust_balm_oracle.py against the
device header compiled for the host, against calculus, and the property the feature exists for -- on a problem with displaced
voxels the robust LM ends closer to the uncontaminated solution than the plain LM does."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_problem

import robust_balm_oracle as rbo
from oracle import balm_oracle as bo

KINDS = ["huber", "softlone", "cauchy", "arctan", "tukey"]
CASE = dict(n_poses=12, n_voxels=150, band=6, seed=7)


def test_numpy_rho_equals_device_header_on_the_host(tmp_path):
    """rho, rho', rho'' of the model against csrc/visual_loss.h (the functions the kernels call) compiled with g++ through
    tests/visual_loss_check.cpp: every kind, scales in metres as the LiDAR stage uses them, s on both sides of a^2, 1e-15
    relative."""
    exe = str(tmp_path / "visual_loss_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "visual_loss_check.cpp"),
                           "-o", exe])
    cases = [(k, a, m * a * a) for k in ["trivial"] + KINDS for a in (0.02, 0.086, 0.37, 1.0)
             for m in (0.0, 1e-6, 0.01, 0.1, 0.5, 0.9, 1.0, 1.1, 2.0, 10.0, 100.0, 1e4)]
    inp = "".join(f"{rbo.KINDS[k]} {float(a).hex()} {float(s).hex()}\n" for k, a, s in cases)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([[float.fromhex(v) for v in line.split()] for line in out if line.strip()])
    ref = np.array([rbo.rho(k, a, s) for k, a, s in cases])
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    err[ref == got] = 0.0
    assert err.max() <= 1e-15, [(cases[i], got[i], ref[i]) for i in np.nonzero(err.max(1) > 1e-15)[0][:5]]


@pytest.mark.parametrize("kind", KINDS)
def test_robust_gradient_matches_finite_differences(kind):
    """Central differences (one Richardson step) of the model's robust cost reproduce its g = sum rho' g_v: the bar and the
    steps of tests/test_oracle.py::test_gradient_and_hessian_match_finite_differences."""
    d = make_problem(8, 30, band=3, seed=21)
    dc, _, a = rbo.contaminated(d)
    prob = rbo.problem(dc)
    x = dc["poses_init"]
    _, g, c, lam, w = rbo.evaluate(prob, x, kind, a)
    assert abs(c - rbo.cost(prob, x, kind, a)) <= 1e-9 * c
    assert w.min() < 1.0 - 1e-3 and w.max() > 0.5         # down-weighted and (nearly) full-weight voxels are both in the sum
    rng = np.random.default_rng(0)
    for _ in range(3):
        dv = rng.standard_normal(6 * 8)

        def d1(h):
            return (rbo.cost(prob, bo.retract(x, h * dv), kind, a) - rbo.cost(prob, bo.retract(x, -h * dv), kind, a)) / (2 * h)

        h = 2e-5
        fd1 = (4 * d1(h / 2) - d1(h)) / 3
        assert abs(fd1 - g @ dv) <= 1e-6 * np.linalg.norm(g) * np.linalg.norm(dv), (kind, fd1, g @ dv)


def test_trivial_is_the_plain_oracle():
    d = make_problem(**CASE)
    prob = rbo.problem(d)
    x = d["poses_init"]
    H, g, c, _, w = rbo.evaluate(prob, x, "trivial", 1.0)
    H0, g0, c0 = bo.acc_evaluate2(prob, x, 0, prob.n_voxels)
    assert np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max() and np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max()
    assert abs(c - c0) <= 1e-12 * c0 and (w == 1.0).all()


def test_cauchy_lm_ends_closer_to_the_clean_solution():
    """Three oracle LMs: the uncontaminated problem, and the contaminated one (a quarter of the voxels with one cluster displaced
    by 5 a .. 20 a) without a loss and with Cauchy at the derived scale a.  Gauge fixed by expressing every pose relative to
    pose 0; distance = largest translation difference.  Only the strict inequality is asserted (figures: DESIGN.md 6.3)."""
    d = make_problem(**CASE)
    dc, touched, a = rbo.contaminated(d)
    hi, lo = rbo.check_input_shares(dc, a)
    x_clean, _ = rbo.damping_iter(rbo.problem(d), d["poses_init"])
    x_plain, _ = rbo.damping_iter(rbo.problem(dc), dc["poses_init"])
    x_cauchy, _ = rbo.damping_iter(rbo.problem(dc), dc["poses_init"], "cauchy", a)
    d_plain, d_cauchy = rbo.gauge_distance(x_plain, x_clean), rbo.gauge_distance(x_cauchy, x_clean)
    print(f"a = {a:.4f} m, above a^2: {hi:.3f}, at or below: {lo:.3f}, plain {d_plain:.4f} m, cauchy {d_cauchy:.4f} m")
    assert d_cauchy < d_plain, (d_cauchy, d_plain)
