"""The reference and the bars of the band-solver tests (tests/band_solve_reference.py), proven on the CPU: the refined reference
agrees with a dense one, a correct blocked LDL^T in numpy meets the bars, and the same code with one planted defect does not.

Systems: H from the C oracle for synth.make_balm_problem(N, 40 N, band=.., loop_frac=0.0, seed=5) at N / band = 400 / 27
(n = 2400, bw = 329) and 171 / 5 (n = 1026, bw = 65), A = H + u diag(diag(H)), u in {0.01, 10}.

What the planted defects reach there (backward, forward error; the C oracle's clean LDL^T: 1.4e-17 .. 3.9e-17 and 7.9e-16 .. 9.2e-15):
    drop_tile    400/27: 1.1e-08, 3.1e-06 (u = 0.01)   3.6e-10, 5.7e-08 (u = 10)     171/5: 1.3e-04, 1.6e-01    1.8e-06, 2.6e-04 (its
                 only non-empty tile is the one next to the diagonal)
    fp32_panel   400/27: 1.2e-11, 5.6e-09              1.9e-12, 1.7e-10             171/5: 2.6e-11, 1.2e-08    3.5e-12, 2.0e-10
    rcp_1e-12    400/27: 3.4e-17, 4.1e-13              6.3e-17, 2.6e-13             171/5: 5.2e-17, 7.1e-13    1.2e-16, 3.1e-13
Every case prints its figures.  The first two defects exceed 1e-10 everywhere.  One reciprocal off by 1e-12 leaves 2.6e-13 at
least, and CAP (5.6e-14) lies halfway, in decades, between that and the 1.2e-14 a correct fp64 LDL^T leaves at worst.

Where the reciprocal defect is planted.  The unknowns come in poses of six, three rotation components and then three translation
components, scaled very differently; in the infinity norm the forward error is carried by the translation components.  The
defect is planted on the first pivot of the middle panel that belongs to a translation component (_translation_pivot).  On a
rotation component the same defect shows in the backward error instead and can leave the forward error at rounding level:
test_reciprocal_defect_on_a_rotation_pivot holds what is true there.
"""
import numpy as np
import pytest

import band_solve_reference as R
from conftest import make_problem

SYSTEMS = [(400, 27), (171, 5)]
US = [0.01, 10.0]
_CACHE = {}


def _system(oracle_mod, N, band, u):
    """(A, b, bw, x_ref, the oracle's two errors): built once per (system, u) and left unchanged."""
    if (N, band) not in _CACHE:
        d = make_problem(N, 40 * N, band=band, loop_frac=0.0, seed=5)
        co = oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"])
        H, g, _ = co.eval_dense(d["poses_init"])
        _CACHE[(N, band)] = (np.array(H), g, R.bandwidth(H))
    if (N, band, u) not in _CACHE:
        H, g, bw = _CACHE[(N, band)]
        A, b = H + u * np.diag(np.diag(H)), -g
        x_ref = R.reference_solve(A, b, bw)
        x_o, rc = oracle_mod.ldlt_solve_dense(A, b)
        assert rc == 0
        _CACHE[(N, band, u)] = (A, b, bw, x_ref, R.errors(A, b, x_o, x_ref))
    return _CACHE[(N, band, u)]


def _translation_pivot(n):
    """The first pivot of band_ldlt_numpy's middle panel whose unknown is a translation component (index mod 6 in 3 .. 5)."""
    k0 = R.NB * (((n + R.NB - 1) // R.NB) // 2)
    return next(k for k in range(k0, k0 + 6) if k % 6 >= 3)


def test_reference_solve_agrees_with_dense_refinement(oracle_mod):
    """n = 660: np.linalg.solve + refinement with a dense np.longdouble residual, against the banded one, to 1e-15."""
    d = make_problem(110, 4400, band=12, loop_frac=0.0, seed=5)
    co = oracle_mod.COracle(110, d["voxel_off"], d["pose_idx"], d["clusters"])
    H, g, _ = co.eval_dense(d["poses_init"])
    for u in US:
        A, b = H + u * np.diag(np.diag(H)), -g
        A_ld, b_ld = A.astype(R.LD), b.astype(R.LD)
        x = np.linalg.solve(A, b).astype(R.LD)
        for _ in range(4):
            x += np.linalg.solve(A, (b_ld - A_ld @ x).astype(np.float64)).astype(R.LD)
        x_ref = R.reference_solve(A, b, R.bandwidth(A))
        assert x_ref.dtype == R.LD
        assert float(np.abs(x_ref - x).max() / np.abs(x).max()) <= 1e-15
        # and the reference is a fixed point of its own refinement: its residual is at the level of the extended format
        be, fe = R.errors(A, b, x_ref, x)
        assert be <= 1e-18 and fe <= 1e-15


def test_errors_of_a_known_perturbation():
    """errors() on a small system with a known answer: x_ref exact, x off by a known relative amount."""
    rng = np.random.default_rng(0)
    A = np.diag(rng.uniform(1, 2, 50)) + 0.01 * rng.standard_normal((50, 50))
    x_ref = rng.standard_normal(50)
    b = (A.astype(R.LD) @ x_ref.astype(R.LD))
    x = x_ref.copy()
    k = int(np.abs(x_ref).argmax())
    x[k] *= 1 + 1e-9
    be, fe = R.errors(A, b, x, x_ref)
    assert abs(fe / 1e-9 - 1) <= 1e-6
    col = np.abs(A[:, k]).max() * abs(x_ref[k]) * 1e-9
    want = col / (np.abs(A).sum(1).max() * np.abs(x).max() + float(np.abs(b).max()))
    assert abs(be / want - 1) <= 1e-6


@pytest.mark.parametrize("u", US)
@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[1]}")
def test_clean_factorisation_meets_the_bars(oracle_mod, system, u):
    """Without a defect: inside CAP, inside K times the oracle's error + 16 eps, and within a small factor of the oracle's.  The
    factor: both are unpivoted fp64 LDL^T factorisations of the same matrix that differ in blocking and summation order only,
    i.e. two draws from the same rounding-error distribution (sums of ~bw terms of relative size eps); 4 x + 16 eps is far more
    than two such draws differ by and far less than any defect above leaves."""
    A, b, bw, x_ref, yard = _system(oracle_mod, *system, u)
    L, rcp = R.band_ldlt_numpy(A, bw)
    assert np.array_equal(np.tril(L), L) and (np.diagonal(L) == 1).all()
    i, j = np.nonzero(L)
    assert (i - j).max() <= bw                                    # no fill outside the band
    got = R.errors(A, b, R.band_ldlt_solve(L, rcp, b), x_ref)
    print(f"clean {system} u={u}: {got[0]:.3e} {got[1]:.3e}  oracle {yard[0]:.3e} {yard[1]:.3e}")
    for e, y in zip(got, yard):
        assert R.within_bars(e, y)
        assert e <= 4 * y + 16 * R.EPS


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("u", US)
@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: f"{s[0]}-{s[1]}")
def test_planted_defect_is_caught(oracle_mod, system, u, defect):
    A, b, bw, x_ref, yard = _system(oracle_mod, *system, u)
    L, rcp = R.band_ldlt_numpy(A, bw, defect, pivot=_translation_pivot(A.shape[0]))
    got = R.errors(A, b, R.band_ldlt_solve(L, rcp, b), x_ref)
    print(f"{defect} {system} u={u}: {got[0]:.3e} {got[1]:.3e}  oracle {yard[0]:.3e} {yard[1]:.3e}")
    assert max(got) > R.CAP
    assert not (R.within_bars(got[0], yard[0]) and R.within_bars(got[1], yard[1]))
    if defect != "rcp_1e-12":
        assert max(got) > 1e-10                                                  # the coarse defects: three decades and more


def test_reciprocal_defect_on_a_rotation_pivot(oracle_mod):
    """171/5, u = 10, the reciprocal defect on the first pivot of the middle panel (column 512, a rotation component): the
    forward error stays under CAP (7.5e-15), but the backward error is 2.5e-15 where the clean factorisation leaves 6.1e-18 --
    a 1e-12 slip against eps = 2.2e-16 rounding.  Held: more than 100 times the clean factorisation's backward error."""
    A, b, bw, x_ref, yard = _system(oracle_mod, 171, 5, 10.0)
    assert (R.NB * ((A.shape[0] + R.NB - 1) // R.NB // 2)) % 6 < 3
    clean = R.errors(A, b, R.band_ldlt_solve(*R.band_ldlt_numpy(A, bw), b), x_ref)
    got = R.errors(A, b, R.band_ldlt_solve(*R.band_ldlt_numpy(A, bw, "rcp_1e-12"), b), x_ref)
    print(f"rcp_1e-12 on a rotation pivot: {got[0]:.3e} {got[1]:.3e}  clean {clean[0]:.3e} {clean[1]:.3e}")
    assert got[0] > 100 * clean[0]
