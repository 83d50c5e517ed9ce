"""CPU tests of the visual stage's robust losses (lvba_visual_set_loss): the reference model (tests/robust_visual_oracle.py)
against calculus and against the plain oracle, the device header compiled for the host against the model, and the C-ABI
additions compiled as C99 and through the adapter."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import robust_visual_oracle as rvo

KINDS = ["huber", "softlone", "cauchy", "arctan", "tukey"]
SCALES = [0.1, 1.0, 2.0]
# multiples of a^2 on both sides of it (not on it: Huber's rho'' jumps there)
GRID = [0.01, 0.1, 0.5, 0.9, 1.1, 2.0, 10.0, 100.0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", SCALES)
def test_loss_derivatives_match_finite_differences(kind, a):
    """Central differences with one Richardson step (error O(h^4)), h = 2e-3 s: small enough for the truncation, large enough
    that rounding stays below 1e-7 where rho'' is tiny next to rho' (Arctan near s = 0)."""
    b = a * a

    def cdiff(k, s, h):
        lo, hi = rvo.rho(kind, a, s - h), rvo.rho(kind, a, s + h)
        return (hi[k] - lo[k]) / (2 * h)

    for m in GRID:
        s = m * b
        h = 2e-3 * s
        r0, r1, r2 = rvo.rho(kind, a, s)
        d1 = (4.0 * cdiff(0, s, h / 2) - cdiff(0, s, h)) / 3.0
        d2 = (4.0 * cdiff(1, s, h / 2) - cdiff(1, s, h)) / 3.0
        if r1 > 0.0:
            assert abs(d1 - r1) <= 1e-7 * abs(r1), (kind, a, m, d1, r1)
        else:                                            # Tukey beyond a^2: rho is flat
            assert d1 == 0.0 and r0 == b / 3.0
        if r2 != 0.0:
            assert abs(d2 - r2) <= 1e-7 * abs(r2), (kind, a, m, d2, r2)
        else:
            assert d2 == 0.0, (kind, a, m, d2)


@pytest.mark.parametrize("kind", KINDS + ["trivial"])
def test_loss_origin_and_concavity(kind):
    """rho(0) = 0, rho'(0) = 1, and rho'' <= 0 everywhere: Ceres' Corrector only ever takes its scaling branch."""
    for a in SCALES:
        assert rvo.rho(kind, a, 0.0)[:2] == (0.0, 1.0)
        for s in np.concatenate([[0.0], np.logspace(-8, 6, 400) * a * a]):
            r0, r1, r2 = rvo.rho(kind, a, s)
            assert r2 <= 0.0 and r1 >= 0.0 and r0 >= 0.0 and r0 <= s * (1 + 1e-6)   # (rounding of 1 + s/a^2 near s = 0)


def _ulps(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ix, iy = x.view(np.int64), y.view(np.int64)
    ix = np.where(ix < 0, np.int64(-2**63) - ix, ix)      # signed-magnitude -> two's complement order
    iy = np.where(iy < 0, np.int64(-2**63) - iy, iy)
    return np.abs(ix - iy)


def test_device_header_matches_model_on_the_host(tmp_path):
    """csrc/visual_loss.h, the functions the kernels call, compiled with g++ (tests/visual_loss_check.cpp): rho, rho', rho''
    within 4 ulp of the model for every kind, on both sides of a^2 and at s = 0."""
    exe = str(tmp_path / "visual_loss_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "visual_loss_check.cpp"),
                           "-o", exe])
    cases = []
    for k in ["trivial"] + KINDS:
        for a in SCALES + [0.37]:
            for m in [0.0, 1e-6] + GRID + [1.0, 1e4]:
                cases.append((k, a, m * a * a))
    inp = "".join(f"{rvo.KINDS[k]} {float(a).hex()} {float(s).hex()}\n" for k, a, s in cases)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([[float.fromhex(v) for v in line.split()] for line in out if line.strip()])
    ref = np.array([rvo.rho(k, a, s) for k, a, s in cases])
    assert got.shape == ref.shape
    worst = _ulps(got, ref)
    assert worst.max() <= 4, [(cases[i], got[i], ref[i]) for i in np.nonzero(worst.max(1) > 4)[0][:5]]


def _problem(synth, **case):
    from oracle import visual_oracle as vo
    d = synth.make_visual_problem(**case)
    return d, vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])


def test_robust_oracle_with_trivial_losses_is_the_oracle(synth):
    """Both families TRIVIAL: the restated loop reproduces VisualOracle.solve() exactly (same trace, same state)."""
    from oracle import visual_oracle as vo
    d, p = _problem(synth, n_cams=6, n_tracks=40, seed=5, invalid_frac=0.3)
    (q0, t0, X0), tr0, st0 = vo.VisualOracle(p).solve()
    (q1, t1, X1), tr1, st1 = rvo.RobustVisualOracle(p, None, ("trivial", 3.0)).solve()
    assert st1 == st0 and tr1 == tr0 and len(tr0) >= 3
    assert np.array_equal(q1, q0) and np.array_equal(t1, t0) and np.array_equal(X1, X0)
    orc = vo.VisualOracle(p)
    assert rvo.RobustVisualOracle(p).cost(*orc.state()) == orc.cost(*orc.state())


def test_robust_oracle_corrects_residuals_and_cost(synth):
    """Huber on displaced observations: the blocks beyond a^2 carry rho(s) in the cost and sqrt(rho') on residual and Jacobian."""
    from oracle import visual_oracle as vo
    d, _ = _problem(synth, n_cams=6, n_tracks=40, seed=5)
    d, mask = rvo.add_outliers(d, 0.15, seed=1)
    p = vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    plain = vo.VisualOracle(p)
    rob = rvo.RobustVisualOracle(p, ("huber", 1.0), ("cauchy", 0.1))
    q, t, X = plain.state()
    r, J = plain.residuals_and_jacobian(q, t, X)
    rt, Jt, s, rho0 = rob.residuals_and_jacobian(q, t, X)
    w = np.sqrt(rob.block_rho(s)[:, 1])[rob.row_block]
    assert np.array_equal(rt, r * w) and np.array_equal(Jt, J * w[:, None])
    fam = rob.block_family
    assert (s[fam == 0] > 1.0).mean() > 0.2                           # a fifth of the blocks beyond the Huber scale
    huber = np.where(s > 1.0, 2.0 * np.sqrt(s) - 1.0, s)
    cauchy = 0.01 * np.log(1.0 + s / 0.01)
    ref = np.where(fam == 0, huber, cauchy)
    assert abs(rob.cost(q, t, X) - 0.5 * ref.sum()) <= 1e-12 * rob.cost(q, t, X)
    assert rob.cost(q, t, X) < plain.cost(q, t, X)


def test_outlier_helper_leaves_synth_untouched(synth):
    d = synth.make_visual_problem(6, 40, seed=5)
    d2, mask = rvo.add_outliers(d, 0.2, seed=3)
    e = synth.make_visual_problem(6, 40, seed=5)
    assert np.array_equal(d["obs_uv"], e["obs_uv"]) and not np.array_equal(d2["obs_uv"], d["obs_uv"])
    disp = np.linalg.norm(d2["obs_uv"] - d["obs_uv"], axis=1)
    assert np.all((disp[mask] >= 20.0 - 1e-9) & (disp[mask] <= 100.0 + 1e-9)) and np.all(disp[~mask] == 0.0)


def test_loss_struct_layout_and_c99_header(pkg, tmp_path):
    """The LVBA_LOSS_* kinds of the header, which stays plain C99, are the package's and the oracle's (lvba_loss's layout:
    tests/test_abi.py)."""
    L = pkg._lib
    src = tmp_path / "loss.c"
    src.write_text('#include <stdio.h>\n#include "lvba_hip.h"\n'
                   'int main(void){printf("%d %d %d %d %d %d\\n", '
                   'LVBA_LOSS_TRIVIAL, LVBA_LOSS_HUBER, LVBA_LOSS_SOFTLONE, LVBA_LOSS_CAUCHY, LVBA_LOSS_ARCTAN, LVBA_LOSS_TUKEY);'
                   'return 0;}\n')
    exe = str(tmp_path / "loss")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v == [L.LOSS_KINDS[k] for k in ["trivial"] + KINDS] == [rvo.KINDS[k] for k in ["trivial"] + KINDS]
    assert {"lvba_visual_set_loss", "lvba_visual_residual_sq"} <= set(L.SYMBOLS)


def test_adapter_compiles_with_and_without_losses(tmp_path):
    """include/lvba_adapter.hpp: optimize_camera_poses_hip keeps its old call form and takes the two loss pointers."""
    src = tmp_path / "adapter_loss.cpp"
    src.write_text(r'''
#include <array>
#include <vector>
#include "lvba_adapter.hpp"
int main() {
    std::vector<std::array<double, 4>> qs(2);
    std::vector<std::array<double, 3>> ts(2), Xs(1);
    std::vector<int64_t> off{0, 0};
    std::vector<int32_t> cam;
    std::vector<double> uv, pl(4, 0.0);
    std::vector<uint8_t> valid{0};
    const double intr[8] = {};
    if (0) {
        lvba::optimize_camera_poses_hip(qs, ts, Xs, off, cam, uv, pl, valid, intr, 0.5, 0.01);
        const lvba_loss hr = lvba::loss_huber(1.0), hp = lvba::loss_huber(0.1);
        lvba::optimize_camera_poses_hip(qs, ts, Xs, off, cam, uv, pl, valid, intr, 0.5, 0.01, nullptr, 0, &hr, &hp);
        const lvba_loss c = lvba::loss_cauchy(2.0);
        lvba::optimize_camera_poses_hip(qs, ts, Xs, off, cam, uv, pl, valid, intr, 0.5, 0.01, nullptr, 0, &c);
    }
    const lvba_loss t = lvba::loss_tukey(3.0);
    return (t.kind == LVBA_LOSS_TUKEY && t.scale == 3.0 && lvba::loss_softlone(1.0).kind == LVBA_LOSS_SOFTLONE &&
            lvba::loss_arctan(1.0).kind == LVBA_LOSS_ARCTAN) ? 0 : 1;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
