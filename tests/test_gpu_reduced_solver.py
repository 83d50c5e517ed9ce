"""The visual stage's reduced camera solve (csrc/bcr.hip, or the band / dense LDL^T of ldlt.hip) against a refined reference, at
the edges of its three kernel families.

What is solved and what it is compared with.  `S, rhs, _ = vp.linearize(q, t, X)`, then `x, solver = vp.solve()`
(lvba_visual_solve: bs_enqueue_solve on the block store the linearisation left on the handle).  lvba_visual_linearize's dense
export copies that block store entry for entry, and nothing rewrites it between the two calls: A = S, b = -rhs built from the
EXPORTED arrays is exactly the system the solver was given (S is the same bits as its transpose, asserted), and the
linearisation's own noise stays out of the comparison.  The reference is band_solve_reference.reference_solve (banded LU with
partial pivoting + refinement in extended precision).

The rows (synth.make_visual_problem(n_cams, 12 n_cams, track_len=.., seed=21); camera half-bandwidth Bb = track_len - 1,
bw = 6 Bb + 5, n = 6 n_cams; all have n <= 1024, so the cameras keep the caller's order): see ROWS.  Every case first asserts
from vp.info() and from `solver` that it landed in the form it is named for.  Which form a system lands in (block_system.hip):
the band store needs bw + 128 < 0.6 n; block cyclic reduction needs the band store, Bb <= 10 and n_cams >= 8 k with
k = max(5, Bb) cameras per block row (32 scalars for k = 5, 64 above); everything else goes to the LDL^T, over the band store or,
without one, over the full lower triangle.  At track_len 4 the band store starts at 42 cameras -- above the 40 that block cyclic
reduction asks for --, so 39, 40 and 41 cameras are solved by the LDL^T over the full triangle, and the smallest systems that
reach the 32-scalar kernels with nb = 8 and nb = 9 are 40 cameras at track_len 2 and 41 at track_len 3.

The bars, on the normwise backward error and on the forward error of every solve.
  Block cyclic reduction (solver 1, 2; bcr_reference.within_bars_bcr): both at most CAP_BCR = (4.8e-12, 2.1e-10) (derived in
    tests/bcr_reference.py, shown in tests/test_bcr_reference_host.py), and both at most K_BCR = 64 times the error the numpy
    restatement of tests/bcr_reference.py leaves on the same system, + 16 eps.  K_BCR is ten times the largest ratio (GPU error /
    restatement error) measured on the MI355X, rounded up to a power of two.  The C oracle's unpivoted LDL^T is no yardstick
    for these rows: the explicit inverses of the diagonal blocks cost about two decades in the backward error.
  LDL^T (solver 0): the backward error is held to band_solve_reference.within_bars unchanged (CAP 5.6e-14, K = 8 times the C
    oracle's unpivoted LDL^T on the same system, + 16 eps).  The forward error is held to the K bar only: on these systems
    cond S[6:, 6:] ~ 1.5e4 and x is small, and the oracle's own forward error (2e-13) already exceeds that CAP.
The sweep (backward: GPU error, ratio to the yardstick; forward: the same):
    n_cams/track_len       solver   backward         forward          yardstick (backward, forward)
    40/2                   1        1.4e-14  0.89    2.2e-12  0.41    1.6e-14  5.4e-12
    41/3                   1        1.4e-14  1.49    9.2e-13  0.64    9.1e-15  1.4e-12
    42/4                   1        3.8e-15  1.03    1.5e-12  4.31    3.7e-15  3.5e-13
    40/4                   0        9.3e-17  1.30    1.3e-13  0.63    7.2e-17  2.1e-13
    41/4                   0        9.9e-17  1.89    1.1e-13  0.93    5.3e-17  1.2e-13
    63/4                   1        8.0e-15  1.10    7.0e-12  4.53    7.3e-15  1.5e-12
    75/2                   1        2.1e-14  1.43    5.7e-12  0.35    1.5e-14  1.6e-11
    85/6                   1        1.3e-14  2.12    3.8e-12  1.48    6.0e-15  2.5e-12
    48/7                   2        8.1e-15  1.49    1.8e-13  2.22    5.4e-15  8.2e-14
    49/7                   2        5.4e-15  1.96    4.4e-13  2.14    2.8e-15  2.0e-13
    80/11                  2        2.4e-14  2.12    7.5e-13  0.23    1.1e-14  3.3e-12
    101/11                 2        2.9e-14  2.42    8.9e-13  0.15    1.2e-14  5.9e-12
    39/4                   0        1.3e-16  1.56    1.6e-13  1.05    8.2e-17  1.5e-13
    47/7                   0        8.9e-17  0.98    9.3e-14  0.59    9.1e-17  1.6e-13
    63/4 LVBA_BCR=0        0        9.5e-17  0.98    2.8e-13  1.92    9.7e-17  1.5e-13
    128/4                  1        3.1e-14  1.31    1.2e-11  0.77    2.3e-14  1.6e-11
    128/4 LVBA_BCR=0       0        1.5e-16  2.51    3.0e-13  0.69    5.8e-17  4.3e-13
    63/4 (fifth solve)     1        8.0e-15  1.10    7.0e-12  4.53    7.3e-15  1.5e-12
Largest ratio of the block-cyclic-reduction rows: 4.53 (63/4, forward) -> K_BCR = 64.  Largest ratio of the LDL^T rows: 2.51 against K = 8.
Every figure is printed by the tests (pytest -s).
"""
import numpy as np
import pytest

import band_solve_reference as R
import bcr_reference as B

pytestmark = pytest.mark.gpu

NB = 64  # LVBA_NB


class Geo:
    """Where a system lands, recomputed from (n_cams, Bb, LVBA_BCR).  A COPY of rules in the solver -- the band-store test of
    bs_build (block_system.hip: band_frac 0.6), bcr_applicable / bcr_block_cams / bcr_pad (csrc/bcr.hip, through their copies in
    tests/bcr_reference.py), ldlt_twist_panels (ldlt.hip).  Only use_band, band_blocks and the solver family can be asserted
    against the handle; whoever changes those rules changes these copies with them, or the rows stop reaching what they are
    named for unnoticed."""

    def __init__(self, M, Bb, bcr_off):
        self.n = 6 * M
        self.bw = 6 * Bb + 5
        self.use_band = self.bw + NB + 64 < 0.6 * self.n
        self.k = B.block_cams(Bb)
        self.nb = -(-M // self.k)
        self.last = M - (self.nb - 1) * self.k          # cameras in the last block row
        bcr = self.use_band and B.applicable(M, Bb) and not bcr_off
        self.solver = 0 if not bcr else 1 if B.pad(self.k) == 32 else 2
        P = (self.n - self.bw) // (2 * NB)
        self.P = P if (P >= 4 and self.use_band) else 0  # panels per end of the two-ended band LDL^T
        self.band_blocks = Bb if self.use_band else M - 1


def _missing_right(nb):
    """Levels at which the last odd row has no right neighbour."""
    return sum(1 for s in sorted({s for s, _ in B.odd_rows(nb)}) if max(i for t, i in B.odd_rows(nb) if t == s) + s >= nb)


# (n_cams, track_len, LVBA_BCR=0?, what the row is there to reach -- asserted on the recomputed table)
ROWS = [
    (40, 2, False, lambda g: g.solver == 1 and g.nb == 8 and g.last == 5),           # smallest 32-scalar system, every level full
    (41, 3, False, lambda g: g.solver == 1 and g.nb == 9 and g.last == 1),           # 2^3 + 1: a top level whose only odd row has no right neighbour
    (42, 4, False, lambda g: g.solver == 1 and g.nb == 9 and g.last == 2 and not Geo(41, 3, False).use_band),  # first band store at track_len 4
    (40, 4, False, lambda g: g.solver == 0 and not g.use_band),                       # LDL^T over the full triangle, n = 240
    (41, 4, False, lambda g: g.solver == 0 and not g.use_band),                       # the last system without a band store
    (63, 4, False, lambda g: g.solver == 1 and g.nb == 13 and g.last == 3 and _missing_right(g.nb) >= 2),
    (75, 2, False, lambda g: g.solver == 1 and g.nb == 15 and g.bw == 11),            # 2^4 - 1; Bb = 1: coupling blocks almost empty
    (85, 6, False, lambda g: g.solver == 1 and g.nb == 17 and g.k == 5 and g.bw == 35),  # Bb = k: the coupling block reaches every camera of the row before
    (48, 7, False, lambda g: g.solver == 2 and g.k == 6 and g.nb == 8),               # 36 real and 28 identity rows
    (49, 7, False, lambda g: g.solver == 2 and g.nb == 9 and g.last == 1),
    (80, 11, False, lambda g: g.solver == 2 and g.k == 10 and g.nb == 8),             # 60 of 64 scalars real
    (101, 11, False, lambda g: g.solver == 2 and g.nb == 11 and g.last == 1),
    (39, 4, False, lambda g: g.solver == 0 and not g.use_band),                       # n = 234, full triangle
    (47, 7, False, lambda g: g.solver == 0 and g.use_band and g.bw == 41 and g.P == 0 and not B.applicable(47, 6)),  # one camera under the 64-scalar threshold
    (63, 4, True, lambda g: g.solver == 0 and g.use_band and g.bw == 23 and g.P == 0),   # band narrower than a tile, one-ended
    (128, 4, False, lambda g: g.solver == 1 and g.nb == 26),
    (128, 4, True, lambda g: g.solver == 0 and g.use_band and g.bw == 23 and g.P == 5),  # two-ended, band narrower than a tile
]
IDS = [f"{M}-{tl}-{'ldlt' if off else 'default'}" for M, tl, off, _ in ROWS]


class Case:
    """One row: the handle, the system it exported, the reference and the yardstick's two errors."""

    def __init__(self, pkg, synth, monkeypatch, oracle_mod, M, track_len, bcr_off):
        if bcr_off:
            monkeypatch.setenv("LVBA_BCR", "0")           # read when the handle lays out its store (the first linearize)
        else:
            monkeypatch.delenv("LVBA_BCR", raising=False)
        d = synth.make_visual_problem(M, 12 * M, track_len=track_len, seed=21)
        self.vp = pkg.VisualProblem(M, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
        self.state = (d["q"], d["t"], d["X"])
        self.S, self.rhs, _ = self.vp.linearize(*self.state)
        self.geo = Geo(M, track_len - 1, bcr_off)
        self.oracle_mod = oracle_mod

    def check_form(self, reach, solver):
        i, g = self.vp.info(), self.geo
        assert reach(g), ("the row's table no longer reaches what it is there for", vars(g))
        assert (i["use_band"], i["band_blocks"], solver) == (int(g.use_band), g.band_blocks, g.solver), (i, solver, vars(g))
        assert np.array_equal(self.S, self.S.T)
        assert R.bandwidth(self.S) <= g.bw
        assert not self.S[:6, 6:].any() and not self.rhs[:6].any()        # camera 0 is constant: a decoupled block

    def system(self):
        """(A, b, x_ref, the yardstick's (backward, forward) errors)."""
        A, b = self.S, -self.rhs
        x_ref = R.reference_solve(A, b, R.bandwidth(A))
        if self.geo.solver == 0:
            x_y, rc = self.oracle_mod.ldlt_solve_dense(A, b)
            assert rc == 0
        else:
            x_y = B.bcr_solve_system(A, b, B.cam_bandwidth(A))
        return A, b, x_ref, R.errors(A, b, x_y, x_ref)


def _hold(tag, solver, A, b, x, x_ref, yard):
    assert np.isfinite(x).all(), tag
    be, fe = R.errors(A, b, x, x_ref)
    print(f"reduced_solver {tag} solver {solver}: backward {be:.3e} (yardstick {yard[0]:.3e}, ratio {be / yard[0]:.2f})  "
          f"forward {fe:.3e} (yardstick {yard[1]:.3e}, ratio {fe / yard[1]:.2f})")
    if solver == 0:
        assert R.within_bars(be, yard[0]), (tag, "backward", be, yard[0])
        assert fe <= R.K * yard[1] + 16 * R.EPS, (tag, "forward", fe, yard[1])
    else:
        assert B.within_bars_bcr(be, yard[0], 0), (tag, "backward", be, yard[0])
        assert B.within_bars_bcr(fe, yard[1], 1), (tag, "forward", fe, yard[1])


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_solve_meets_refined_reference(pkg, synth, monkeypatch, oracle_mod, row):
    M, track_len, bcr_off, reach = row
    c = Case(pkg, synth, monkeypatch, oracle_mod, M, track_len, bcr_off)
    try:
        x, solver = c.vp.solve()
        c.check_form(reach, solver)
        A, b, x_ref, yard = c.system()
        _hold(f"{M}/{track_len}{' LVBA_BCR=0' if bcr_off else ''}", solver, A, b, x, x_ref, yard)
    finally:
        c.vp.close()


def test_repeated_solves_on_one_handle(pkg, synth, monkeypatch, oracle_mod):
    """Five solves of 63 / 4 (32-scalar block rows, nb = 13) on one handle.  enqueue_solve_launches (block_system.hip) captures
    the launch sequence of solve_launches into a graph at the handle's third solve, and the block-cyclic-reduction path is
    captured like the LDL^T: the status memset, bcr_assemble_kernel, the four bcr_level_kernel launches and
    bcr_back_all_kernel; solves three to five are replays.  The sentinel refill of x (bcr_assemble_kernel) and the parity of the
    two L arrays (every solve starts reading L and writing L2) must survive that: all five results are the same bits, and the
    last one holds the bars."""
    c = Case(pkg, synth, monkeypatch, oracle_mod, 63, 4, False)
    try:
        out = [c.vp.solve() for _ in range(5)]
        c.check_form(lambda g: g.solver == 1 and g.nb == 13, out[0][1])
        for x, solver in out[1:]:
            assert solver == out[0][1] and np.array_equal(x, out[0][0])
        A, b, x_ref, yard = c.system()
        _hold("63/4 (fifth solve)", out[4][1], A, b, out[4][0], x_ref, yard)
    finally:
        c.vp.close()


def test_solve_needs_a_linearisation(pkg, synth, monkeypatch, oracle_mod):
    """LVBA_ERR_STATE before the first linearize and after a refine (which replaces the system on the handle)."""
    c = Case(pkg, synth, monkeypatch, oracle_mod, 42, 4, False)
    d = synth.make_visual_problem(42, 12 * 42, track_len=4, seed=21)
    fresh = pkg.VisualProblem(42, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    try:
        with pytest.raises(pkg._lib.LvbaError) as e:
            fresh.solve()
        assert e.value.code == pkg._lib.ERR_STATE
        x, _ = c.vp.solve()
        c.vp.refine(*c.state, max_iter=1)
        with pytest.raises(pkg._lib.LvbaError) as e:
            c.vp.solve()
        assert e.value.code == pkg._lib.ERR_STATE
        c.vp.linearize(*c.state)
        assert np.array_equal(c.vp.solve()[0], x)
    finally:
        fresh.close()
        c.vp.close()
