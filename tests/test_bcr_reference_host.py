"""The restatement and the bars of the reduced-solver tests (tests/bcr_reference.py), proven on the CPU: the padded block cyclic
reduction in numpy meets the bars on two reduced camera systems, and the same code with one planted defect does not.

Systems: synth.make_visual_problem(41, 492, track_len=4, seed=21) -- block rows of 32 scalars, nb = 9 = 2^3 + 1, the last block
row holds one camera -- and (48, 576, track_len=7, seed=21) -- block rows of 64 scalars, k = 6, nb = 8 --, linearised on the CPU
with oracle.visual_oracle: Jacobi scaling, the LM diagonal at radius 1e4, the Schur complement over the landmarks.  Camera 0 is
constant: its decoupled block (the 1e-10 LM diagonal alone, zero right-hand side) goes in front, as lvba_visual_linearize
exports it.  The solver's sign: x = -S^-1 rhs.

What is measured there (backward, forward error; every case prints its figures):
    honest restatement        41/4: 3.2e-15, 1.4e-13          48/7: 5.8e-15, 1.1e-13
    oracle's unpivoted LDL^T  41/4: 6.2e-17, 1.5e-13          48/7: 8.4e-17, 1.7e-13
    inv_fp32, least over every odd row   41/4: 4.0e-09, 3.1e-07 (the last odd row: one camera)    48/7: 3.7e-08, 2.9e-06
    drop_q, stale_L           backward >= 1.8e-5, forward >= 6.7e-2 at every placement tried
    keep_L                    the honest bits: the only row without r - 2 s is row 0, which has no left neighbour, so its new
                              coupling block is zero anyway and nobody reads it (csrc/bcr.hip: keepl == hasl)
"""
import importlib

import numpy as np
import pytest

import bcr_reference as B

SYSTEMS = [(41, 492, 4), (48, 576, 7)]
_CACHE = {}


def reduced_system(n_cams, n_tracks, track_len, radius=1e4):
    """(S [6M, 6M] exactly symmetric, b = -rhs [6M]) of the visual problem at its initial point, in the caller's camera order."""
    from oracle import visual_oracle as vo
    synth = importlib.import_module("global-lvba_amd.synth")
    d = synth.make_visual_problem(n_cams, n_tracks, track_len=track_len, seed=21)
    orc = vo.VisualOracle(vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"],
                                           d["valid"], d["intr"]))
    r, J = orc.residuals_and_jacobian(*orc.state())
    J = J / (1.0 + np.sqrt((J * J).sum(0)))
    D2 = np.clip((J * J).sum(0), 1e-6, 1e32) / radius
    A = J.T @ J + np.diag(D2)
    g = J.T @ r
    nc, T = orc.n_cam, len(orc.act)
    Bc, E = A[:nc, :nc], A[:nc, nc:]
    Ci = np.zeros((3 * T, 3 * T))
    for i in range(T):
        s = slice(3 * i, 3 * i + 3)
        Ci[s, s] = np.linalg.inv(A[nc:, nc:][s, s])
    Sr = Bc - E @ Ci @ E.T
    S = np.zeros((nc + 6, nc + 6))
    S[:6, :6] = (1e-6 / radius) * np.eye(6)                     # min_lm_diagonal / radius
    S[6:, 6:] = 0.5 * (Sr + Sr.T)
    rhs = np.concatenate([np.zeros(6), g[:nc] - E @ (Ci @ g[nc:])])
    return S, -rhs


def _system(n_cams, n_tracks, track_len):
    """(S, b, Bb, x_ref, the honest restatement's two errors): built once and left unchanged."""
    key = (n_cams, n_tracks, track_len)
    if key not in _CACHE:
        S, b = reduced_system(*key)
        Bb = B.cam_bandwidth(S)
        x_ref = B.reference_solve(S, b, B.bandwidth(S))
        honest = B.errors(S, b, B.bcr_solve_system(S, b, Bb), x_ref)
        _CACHE[key] = (S, b, Bb, x_ref, honest)
    return _CACHE[key]


def _nb(S, Bb):
    return -(-(S.shape[0] // 6) // B.block_cams(Bb))


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[2]}")
def test_padding_holds_the_system(system):
    """assemble(): the block rows put back together are S on the cameras' scalars and the identity on the padding; the forms the
    two systems are there for (32 / 64 scalars, a last row of one camera / 36 real and 28 identity rows)."""
    S, b, Bb, _, _ = _system(*system)
    M = S.shape[0] // 6
    assert Bb == system[2] - 1 and B.applicable(M, Bb)
    D, L, rhs, k = B.assemble(S, b, Bb)
    nb, BP = rhs.shape
    assert (k, BP, nb) == ((5, 32, 9) if system[2] == 4 else (6, 64, 8))
    full = np.zeros((nb * BP, nb * BP))
    for R in range(nb):
        full[R * BP:(R + 1) * BP, R * BP:(R + 1) * BP] = D[R]
        if R:
            full[R * BP:(R + 1) * BP, (R - 1) * BP:R * BP] = L[R]
            full[(R - 1) * BP:R * BP, R * BP:(R + 1) * BP] = L[R].T
    real = np.concatenate([R * BP + np.arange(6 * (min((R + 1) * k, M) - R * k)) for R in range(nb)])
    assert len(real) == 6 * M and np.array_equal(full[np.ix_(real, real)], S)
    padding = np.setdiff1d(np.arange(nb * BP), real)
    assert np.array_equal(full[np.ix_(padding, padding)], np.eye(len(padding)))
    assert not full[np.ix_(padding, real)].any() and not rhs.reshape(-1)[padding].any()
    assert np.array_equal(B.scatter(rhs, M, k), b)
    if system[2] == 4:
        assert 6 * (M - (nb - 1) * k) == 6                                      # the last block row holds one camera
    else:
        assert 6 * k == 36 and BP - 6 * k == 28


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[2]}")
def test_honest_restatement_meets_the_bars(oracle_mod, system):
    """Inside CAP_BCR on both measures (the K bar compares with this very figure).  The oracle's unpivoted LDL^T on the same
    system is printed beside it: about two decades better in the backward error, which is why it is no yardstick for BCR."""
    S, b, Bb, x_ref, honest = _system(*system)
    x_o, rc = oracle_mod.ldlt_solve_dense(S, b)
    assert rc == 0
    ldlt = B.errors(S, b, x_o, x_ref)
    print(f"honest {system}: {honest[0]:.3e} {honest[1]:.3e}   oracle LDL^T {ldlt[0]:.3e} {ldlt[1]:.3e}")
    for m in (0, 1):
        assert B.within_bars_bcr(honest[m], honest[m], m)
    assert honest[0] > 10 * ldlt[0]


@pytest.mark.parametrize("place", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("defect", ["inv_fp32", "drop_q", "stale_L"])
@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[2]}")
def test_planted_defect_is_caught(system, defect, place):
    """One defect at the first, a middle and the last odd row (drop_q: of the odd rows that have a right neighbour; stale_L: at
    that row's level): both measures leave the bars."""
    S, b, Bb, x_ref, honest = _system(*system)
    where = B.placements(_nb(S, Bb), need_right=defect == "drop_q")[place]
    got = B.errors(S, b, B.bcr_solve_system(S, b, Bb, defect, where), x_ref)
    print(f"{defect} {system} at (s, i) = {where}: {got[0]:.3e} {got[1]:.3e}   honest {honest[0]:.3e} {honest[1]:.3e}")
    for m in (0, 1):
        assert got[m] > B.CAP_BCR[m]
        assert not B.within_bars_bcr(got[m], honest[m], m)


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[2]}")
def test_keep_L_changes_nothing(system):
    """The new coupling block of a row without r - 2 s: that row is row 0 at every level (an even row r = 2 m s with a left
    neighbour has m >= 1), row 0 has no left neighbour, so what it would write is zero and no level reads L_0.  Planted at every
    level, the defect returns the honest bits: the condition `r - 2 s >= 0` of the kernels (keepl) repeats `hasl`."""
    S, b, Bb, _, _ = _system(*system)
    want = B.bcr_solve_system(S, b, Bb)
    for s in sorted({s for s, _ in B.odd_rows(_nb(S, Bb))}):
        assert np.array_equal(B.bcr_solve_system(S, b, Bb, "keep_L", (s, s)), want)


def test_cap_lies_halfway():
    """CAP_BCR per measure is the geometric mean of HONEST_WORST and INV_FP32_LEAST, and those two are what is measured here:
    the worst honest error over the two systems and the least inv_fp32 error over EVERY odd row of both.  The recorded figures
    are held to a factor of four: the honest ones are rounding noise that moves with the BLAS underneath numpy, and a factor of
    four on either end moves the halfway point by 0.3 of the three decades that separate it from both."""
    worst, least = [0.0, 0.0], [np.inf, np.inf]
    for system in SYSTEMS:
        S, b, Bb, x_ref, honest = _system(*system)
        for where in B.odd_rows(_nb(S, Bb)):
            got = B.errors(S, b, B.bcr_solve_system(S, b, Bb, "inv_fp32", where), x_ref)
            print(f"inv_fp32 {system} at {where}: {got[0]:.3e} {got[1]:.3e}")
            least = [min(a, g) for a, g in zip(least, got)]
        worst = [max(a, h) for a, h in zip(worst, honest)]
    print(f"honest worst {worst[0]:.3e} {worst[1]:.3e}   inv_fp32 least {least[0]:.3e} {least[1]:.3e}   "
          f"CAP_BCR {B.CAP_BCR[0]:.3e} {B.CAP_BCR[1]:.3e}")
    for m in (0, 1):
        assert B.HONEST_WORST[m] / 4 <= worst[m] <= B.HONEST_WORST[m] * 4
        assert B.INV_FP32_LEAST[m] / 4 <= least[m] <= B.INV_FP32_LEAST[m] * 4
        assert abs(np.log10(B.CAP_BCR[m]) - 0.5 * (np.log10(B.HONEST_WORST[m]) + np.log10(B.INV_FP32_LEAST[m]))) <= 1e-12
        assert worst[m] * 100 < B.CAP_BCR[m] < least[m] / 100
