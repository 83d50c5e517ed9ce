"""The damped band solve (ldlt.hip and its headers) against a refined reference, at the edges of its launch schedule.

What is solved and what it is compared with.  `H, g, _ = prob.eval(x0)`, then `dx = prob.solve(u)`.  lvba_balm_eval's dense
export (export_dense_kernel / export_vec_kernel) copies, entry for entry and without arithmetic, the block store `bs.Hblk()` /
`bs.g()` that the solve's fill kernels (ldlt_prepare_band_kernel, ldlt_prepare_kernel) read, and neither is rewritten between
the two calls: so A = H + u diag(diag(H)), b = -g built from the EXPORTED H and g is exactly the system the solver was given,
and the evaluation's own noise (~1e-9 against the oracle's Hessian, checked in test_gpu_balm.py) stays out of the comparison.
The reference is band_solve_reference.reference_solve (banded LU with partial pivoting + refinement in extended precision).

The bars (band_solve_reference.within_bars), on the normwise backward error and on the forward error of every solve:
    both at most CAP = 5.6e-14 (derived in tests/band_solve_reference.py, shown in tests/test_band_solve_reference_host.py), and
    both at most K = 8 times the error the C oracle's unpivoted LDL^T (oracle.ldlt_solve_dense) leaves on the same system, + 16 eps.
K is ten times the largest ratio (GPU error / oracle error) measured on the MI355X, rounded up to a power of two.  The sweep
(backward: GPU error, ratio; forward: GPU error, ratio).  Default form, band store unless "dense":
    N/band   u      backward         forward          |  N/band          u      backward         forward
    110/12   0.01   3.4e-18  0.22    2.1e-15  0.11    |  352/16          0.01   3.5e-18  0.23    1.6e-15  0.24
    110/12   10     5.2e-18  0.30    5.0e-16  0.20    |  352/16          10     5.5e-18  0.24    4.0e-16  0.31
    128/12   0.01   4.1e-18  0.21    2.2e-15  0.24    |  400/27          0.01   3.7e-18  0.25    2.2e-15  0.26
    128/12   10     8.2e-18  0.23    3.3e-16  0.23    |  400/27          10     1.3e-17  0.35    3.9e-16  0.18
    153/12   0.01   6.8e-18  0.48    3.0e-15  0.18    |  300/48          0.01   5.0e-18  0.15    3.9e-15  0.17
    153/12   10     6.8e-18  0.24    5.5e-16  0.28    |  300/48          10     4.6e-18  0.08    7.1e-16  0.21
    174/12   0.01   6.1e-18  0.44    3.1e-15  0.28    |  300/48 dense    0.01   6.3e-18  0.19    2.6e-15  0.11
    174/12   10     4.2e-18  0.16    6.3e-16  0.78    |  300/48 dense    10     7.7e-18  0.14    5.4e-16  0.16
    171/5    0.01   3.9e-18  0.50    4.8e-15  0.41    |  352/16 dense    0.01   4.1e-18  0.27    2.3e-15  0.33
    171/5    10     5.6e-18  0.47    4.9e-16  0.41    |  352/16 dense    10     7.5e-18  0.32    4.4e-16  0.34
The LVBA_SOLVER forms (one child process each; "default" repeats the rows above from a child):
    400/27 form      u      backward         forward          |  300/48 form      u      backward         forward
    default          0.01   3.7e-18  0.25    2.2e-15  0.26    |  default          0.01   5.0e-18  0.15    3.9e-15  0.17
    default          10     1.3e-17  0.35    3.9e-16  0.18    |  default          10     4.6e-18  0.08    7.1e-16  0.21
    bulk64           0.01   3.7e-18  0.25    2.2e-15  0.26    |  bulk64           0.01   5.0e-18  0.15    3.9e-15  0.17
    bulk64           10     1.3e-17  0.35    3.9e-16  0.18    |  bulk64           10     4.6e-18  0.08    7.1e-16  0.21
    nodefer          0.01   3.6e-18  0.25    2.2e-15  0.26    |  nodefer          0.01   3.5e-18  0.11    3.3e-15  0.14
    nodefer          10     1.3e-17  0.35    3.9e-16  0.18    |  nodefer          10     4.6e-18  0.08    7.1e-16  0.21
    bulk64,nodefer   0.01   3.6e-18  0.25    2.2e-15  0.26    |  bulk64,nodefer   0.01   3.5e-18  0.11    3.3e-15  0.14
    bulk64,nodefer   10     1.3e-17  0.35    3.9e-16  0.18    |  bulk64,nodefer   10     4.6e-18  0.08    7.1e-16  0.21
    notwist          0.01   3.1e-18  0.21    2.0e-15  0.23    |  notwist          0.01   6.3e-18  0.19    2.6e-15  0.11
    notwist          10     1.3e-17  0.35    4.7e-16  0.21    |  notwist          10     7.7e-18  0.14    5.4e-16  0.16
Largest ratio: 0.78 -> K = 8.  The oracle's own errors on these systems: backward 7.7e-18 .. 5.5e-17, forward 8.1e-16 .. 2.3e-14
(300/48, u = 0.01).  Every figure is printed by the tests (pytest -s).

The rows (synth.make_balm_problem(N, 40 N, band=.., loop_frac=0.0, seed=5); block half-bandwidth Bb = 2 band, bw = 6 Bb + 5,
T = ceil(bw / 64) tile rows below a panel, P = (n - bw) // 128 panels per end, two ends if P >= 4, middle block S = n - 128 P):
see ROWS; every case first asserts from prob.info() that it landed in the form it was chosen for.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import band_solve_reference as R
from conftest import make_problem

pytestmark = pytest.mark.gpu

NB = 64  # LVBA_NB


# _pair_split and Geo are COPIES of rules in the solver -- the cs / Tb split and is_e of ldlt_schedule_phase (ldlt_schedule.h),
# ldlt_twist_panels (ldlt.hip).  Only twist_panels can be asserted against lvba_balm_info; the split is not exported.  Whoever
# changes those rules changes these copies with them, or the rows stop reaching the launches they are named for unnoticed.
def _pair_split(T):
    """(cs, Tb) of a pair of panels with T tile rows below them: the pair's rank-128 update covers bulk tile columns [1, Tb);
    [1, cs) go into one launch and, if cs < Tb, [cs, Tb) into the next."""
    Tb = T - 1
    items = lambda c: (Tb - c + 1) // 2
    tot = sum(items(c) for c in range(1, Tb))
    part, cs = 0, 1
    while cs < Tb and (cs < 3 or 2 * part < tot):
        part += items(cs)
        cs += 1
    return cs, Tb


class Geo:
    """The table of the module docstring, recomputed from a block half-bandwidth."""

    def __init__(self, N, Bb):
        self.n = 6 * N
        self.bw = 6 * Bb + 5
        self.T = -(-self.bw // NB)
        P = (self.n - self.bw) // (2 * NB)
        self.P = P if P >= 4 else 0          # ldlt_twist_panels
        self.S = self.n - 2 * NB * self.P
        self.paired = self.T >= 3            # is_e: T(e) >= 3, T(e + 1) >= 2
        self.cs, self.Tb = _pair_split(self.T)


# (N, band, what the row is there to reach -- asserted on the recomputed table)
ROWS = [
    (110, 12, lambda g: g.P == 0 and g.n % NB == 20),                      # band store, plain top-down (too short for two ends)
    (128, 12, lambda g: g.P == 4 and g.n % NB == 0),                       # smallest two-ended system, every panel full
    (153, 12, lambda g: g.P > 0 and g.S == g.bw + 1),                      # smallest possible middle block
    (174, 12, lambda g: g.P > 0 and g.S == g.bw + 127 and g.n > 1024),     # largest possible middle block; ordering computed
    (171, 5, lambda g: g.bw == NB + 1 and not g.paired and g.P % 2 == 1 and (g.n - NB * g.P) % NB == 2),  # one column over a tile
    (352, 16, lambda g: g.paired and g.cs == g.Tb and g.P > 0 and g.P % 2 == 0),   # pairing without a second half, even P
    (400, 27, lambda g: g.paired and g.cs < g.Tb and g.P > 0),             # pair update split over two launches
    (300, 48, lambda g: g.T == 10 and g.cs < g.Tb and g.P % 2 == 1),       # wide band, odd P: unpaired last panel closes the phase
]
REACH = {(N, band): f for N, band, f in ROWS}
CASES = [(N, band, "band") for N, band, _ in ROWS] + [(300, 48, "dense"), (352, 16, "dense")]
US = [0.01, 10.0]



class Row:
    """One (N, band, store): the handle, the system it exported, and per u the reference and the oracle's two errors."""

    def __init__(self, pkg, N, band, store):
        self.N, self.band, self.store = N, band, store
        d = make_problem(N, 40 * N, band=band, loop_frac=0.0, seed=5)
        kw = dict(band_frac=0.0) if store == "dense" else {}
        self.prob = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"], **kw)
        self.H, self.g, _ = self.prob.eval(d["poses_init"])
        self.info = self.prob.info()
        self.bw = R.bandwidth(self.H)            # of the exported matrix, in the caller's pose order
        self.sys = {}

    def check_form(self):
        i, geo = self.info, Geo(self.N, 2 * self.band)
        assert REACH[(self.N, self.band)](geo), ("the row's table no longer reaches what it is there for", vars(geo))
        if self.store == "dense":
            assert (i["use_band"], i["band_blocks"], i["twist_panels"]) == (0, self.N - 1, 0), i
        else:
            assert (i["use_band"], i["band_blocks"], i["twist_panels"]) == (1, 2 * self.band, geo.P), (i, vars(geo))
        assert self.bw <= geo.bw
        return geo

    def system(self, oracle_mod, u):
        """(A, b, x_ref, yardstick), computed once per u."""
        A = self.H + u * np.diag(np.diag(self.H))
        b = -self.g
        if u not in self.sys:
            x_ref = R.reference_solve(A, b, self.bw)
            x_o, rc = oracle_mod.ldlt_solve_dense(A, b)
            assert rc == 0
            self.sys[u] = (x_ref, R.errors(A, b, x_o, x_ref))
        return (A, b) + self.sys[u]


@pytest.fixture(scope="module")
def rows(pkg):
    """rows(N, band, store) -> Row, built on first use; every handle is closed when the module is done."""
    made = {}

    def get(N, band, store):
        if (N, band, store) not in made:
            made[(N, band, store)] = Row(pkg, N, band, store)
        return made[(N, band, store)]

    yield get
    for r in made.values():
        r.prob.close()


def _hold(tag, A, b, dx, x_ref, yard):
    assert np.isfinite(dx).all(), tag
    be, fe = R.errors(A, b, dx, x_ref)
    print(f"band_solver {tag}: backward {be:.3e} (oracle {yard[0]:.3e}, ratio {be / yard[0]:.2f})  "
          f"forward {fe:.3e} (oracle {yard[1]:.3e}, ratio {fe / yard[1]:.2f})")
    assert R.within_bars(be, yard[0]), (tag, "backward", be, yard[0])
    assert R.within_bars(fe, yard[1]), (tag, "forward", fe, yard[1])


@pytest.mark.parametrize("u", US)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_solve_meets_refined_reference(rows, oracle_mod, case, u):
    c = rows(*case)
    c.check_form()
    A, b, x_ref, yard = c.system(oracle_mod, u)
    dx = c.prob.solve(u)
    _hold(f"{case[0]}/{case[1]} {case[2]} u={u}", A, b, dx, x_ref, yard)


def test_repeated_solves_on_one_handle(rows, oracle_mod):
    """solve(0.01), solve(10), solve(0.01): the replayed graph with a new damping value, on a band store whose never-rewritten
    part must still read as zero -- the first and third results are the same bits, the second holds the bars."""
    c = rows(400, 27, "band")
    c.check_form()
    first, second, third = c.prob.solve(0.01), c.prob.solve(10.0), c.prob.solve(0.01)
    assert np.array_equal(first, third)
    A, b, x_ref, yard = c.system(oracle_mod, 10.0)
    _hold("400/27 band u=10.0 (between two solves with 0.01)", A, b, second, x_ref, yard)
    A, b, x_ref, yard = c.system(oracle_mod, 0.01)
    _hold("400/27 band u=0.01 (third solve)", A, b, third, x_ref, yard)


def _pinned_solver_doubles(n, bw, band):
    """The LDL^T's store + workspace in doubles as every handle has had them (the literal rules that
    tests/ldlt_layout_check.cpp pins csrc/ldlt_layout.h to); bw: the half-bandwidth in scalars, band: the storage form."""
    if band:
        ldab = bw + NB + 64
        store = 2 * (ldab * (n + 1)) + 65 * ldab
    else:
        store, bw = n * n + 64 * n + 128, n - 1
    ldz = min(bw + NB + 64, n)
    one = -(-n // NB) * 4096 + 3 * n + 4 * ldz * NB + 64 + 2 * 4096 + 2 * 4096
    return store + 2 * one + n + 64 + (min(n, bw + 2 * NB) * (bw + 2) + 64) + 8


def test_handle_memory_is_the_pinned_layout(rows):
    """The smallest row (110/12) in band and in dense storage: the two handles are built from the same problem in the same
    pose order (n <= 1024: no reordering) and differ in the Hessian store (hess_bytes) and in the solver's store and
    workspace only, so the difference of their device_bytes must be exactly what the pinned size rules give.  That holds
    only if every allocation site goes through the layout header and a handle takes the memory it always took."""
    N, band, _ = ROWS[0]
    assert (N, band) == min((r[0], r[1]) for r in ROWS)
    b, d = rows(N, band, "band"), rows(N, band, "dense")
    n, bw = 6 * N, 6 * (2 * band) + 5
    assert (b.info["use_band"], b.info["band_blocks"]) == (1, 2 * band) and (d.info["use_band"], d.info["band_blocks"]) == (0, N - 1)
    assert b.info["hess_bytes"] == 8 * N * (2 * band + 1) * 36 and d.info["hess_bytes"] == 8 * N * N * 36
    want = b.info["hess_bytes"] - d.info["hess_bytes"] + 8 * (_pinned_solver_doubles(n, bw, True) - _pinned_solver_doubles(n, bw, False))
    got = b.info["device_bytes"] - d.info["device_bytes"]
    print(f"band_solver memory {N}/{band}: band {b.info['device_bytes']} dense {d.info['device_bytes']} difference {got} pinned {want}")
    assert got == want


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("global-lvba_amd")
synth = importlib.import_module("global-lvba_amd.synth")
N, band = int(sys.argv[3]), int(sys.argv[4])
d = synth.make_balm_problem(N, 40 * N, band=band, loop_frac=0.0, seed=5)
prob = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"])
_, g, _ = prob.eval(d["poses_init"], want_H=False)
i = prob.info()
np.savez(sys.argv[2], g=g, dx=np.stack([prob.solve(float(u)) for u in sys.argv[5:]]),
         form=np.array([i["use_band"], i["band_blocks"], i["twist_panels"]]))
"""
FORMS = ["", "bulk64", "nodefer", "bulk64,nodefer", "notwist"]
_child_failed = []


@pytest.mark.parametrize("row", [(400, 27), (300, 48)], ids=lambda r: f"{r[0]}-{r[1]}")
def test_every_form_meets_the_reference(rows, oracle_mod, tmp_path, row):
    """One child process per LVBA_SOLVER form (the switches are read once per process).  Each child evaluates and solves on its
    own; its g must be the parent's bits -- then it solved the parent's system -- and its dx is held to the same bars against
    the one reference.  No child is started after one that exited non-zero or ran into its time limit."""
    assert not _child_failed, f"an earlier child failed, none is started after it: {_child_failed}"
    N, band = row
    c = rows(N, band, "band")
    geo = c.check_form()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    for k, form in enumerate(FORMS):
        out = tmp_path / f"form_{k}.npz"
        env = dict(os.environ)
        env.pop("LVBA_SOLVER", None)
        if form:
            env["LVBA_SOLVER"] = form
        try:
            r = subprocess.run([sys.executable, str(script), root, str(out), str(N), str(band)] + [repr(u) for u in US],
                               env=env, capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            _child_failed.append((row, form, "time limit"))
            raise
        if r.returncode != 0:
            _child_failed.append((row, form, r.returncode))
        assert r.returncode == 0, (form, r.returncode, r.stderr[-2000:])
        z = np.load(out)
        assert np.array_equal(z["g"], c.g), form
        assert z["form"].tolist() == [1, 2 * band, 0 if "notwist" in form else geo.P], (form, z["form"])
        for j, u in enumerate(US):
            A, b, x_ref, yard = c.system(oracle_mod, u)
            _hold(f"{N}/{band} form '{form or 'default'}' u={u}", A, b, z["dx"][j], x_ref, yard)
