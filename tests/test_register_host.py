"""CPU tests of the scan-to-map registration (lvba_register_*): the device header (csrc/register_device.h) compiled for the
host against the numpy restatement (tests/register_oracle.py), the restatement's Jacobian against central differences of the
residual along the retraction, the conditions on the shared fixture, and the struct layouts."""
import ctypes
import importlib

import numpy as np
import pytest

from host_build import build_check

import register_cases as rc
import register_oracle as ro


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("register_check", tmp_path_factory.mktemp("emul_register")))
    f64 = np.ctypeslib.ndpointer(np.float64, flags="C")
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
    lib.emul_linearize.argtypes = [ctypes.c_int64, f32, f64, f64, u8, ctypes.c_double, ctypes.c_int, ctypes.c_double, f64, f64, f64, u8]
    lib.emul_linearize.restype = None
    lib.emul_step.argtypes = [f64, ctypes.c_double, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, f64,
                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.emul_jacobi_min.argtypes = [f64, ctypes.c_int]
    lib.emul_jacobi_min.restype = ctypes.c_double
    lib.emul_ldlt_solve.argtypes = [f64, f64, ctypes.c_int]
    return lib


def host_linearize(emul, T, P, lin, gate, loss=None):
    P = np.ascontiguousarray(P, np.float32)
    sums, W, r, inl = np.zeros(29), np.zeros((len(P), 3)), np.zeros(len(P)), np.zeros(len(P), np.uint8)
    kind = 0 if loss is None else {"huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}[loss[0]]
    emul.emul_linearize(len(P), P, np.ascontiguousarray(T, np.float64), np.ascontiguousarray(lin["plane"]),
                        lin["found"].astype(np.uint8), gate, kind, 0.0 if loss is None else float(loss[1]), sums, W, r, inl)
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(ro.TRI):
        H[a, b] = H[b, a] = sums[k]
    return dict(H=H, g=sums[21:27].copy(), cost=sums[27], inliers=int(sums[28]), W=W, r=r, inl=inl > 0, sums=sums)


def relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


@pytest.mark.parametrize("which", ["truth", "start"])
@pytest.mark.parametrize("loss", [None, ("cauchy", 0.03), ("huber", 0.02), ("tukey", 0.05)])
def test_host_linearisation_matches_oracle(emul, which, loss):
    """The per-point rule of the device header, summed in index order, against the oracle's matrix products: 1e-12 relative."""
    T = {"truth": rc.truth, "start": rc.start}[which]()
    P = rc.query_points()
    lin = rc.oracle_linearize(which) if loss is None else ro.linearize(rc.oracle_map(), rc.VS, T, P, rc.GATE, loss)
    got = host_linearize(emul, T, P, lin, rc.GATE, loss)
    assert np.array_equal(got["W"], ro.world_points(T, P))                  # the stated operation order, bit for bit
    assert np.array_equal(got["inl"], lin["inl"]) and got["inliers"] == lin["inliers"] > 500
    assert np.array_equal(got["r"][lin["found"]], lin["r"][lin["found"]])
    assert relmax(got["H"], lin["H"]) <= 1e-12 and relmax(got["g"], lin["g"]) <= 1e-12
    assert abs(got["cost"] - lin["cost"]) <= 1e-12 * lin["cost"]


def test_oracle_jacobian_is_the_derivative_along_the_retraction():
    """J against central differences of r(retract(T, h e_k)) with the association held fixed; r is linear in t and smooth in theta,
    so the error of the difference quotient is h^2 |p| / 6 ~ 1e-9 at h = 1e-5 plus rounding 1e-16 |w| / h ~ 1e-10."""
    T, P = rc.start(), rc.query_points()
    lin = rc.oracle_linearize("start")
    f = lin["found"]
    h = 1e-5
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        rp = ro.residuals(ro.retract(T, e), P, lin["plane"])[0]
        rm = ro.residuals(ro.retract(T, -e), P, lin["plane"])[0]
        assert np.abs((rp - rm)[f] / (2 * h) - lin["J"][f, k]).max() <= 1e-8


def test_host_step_matches_oracle(emul):
    """One step of the device header from the oracle's sums: same state, eigenvalue, step and retracted pose as numpy's."""
    T, P = rc.start(), rc.query_points()
    lin = rc.oracle_linearize("start")
    got = host_linearize(emul, T, P, lin, rc.GATE)
    me, rm = ctypes.c_double(), ctypes.c_double()
    T1 = T.copy()
    o = rc.OPTS
    st = emul.emul_step(got["sums"], o["max_distance"], o["min_inliers"], o["min_eigenvalue"], o["tol_rot"], o["tol_pos"], T1,
                        ctypes.byref(me), ctypes.byref(rm))
    assert st == -1                                                         # goes on
    ev = np.linalg.eigvalsh(lin["H"] / lin["inliers"])
    assert abs(me.value - ev[0]) <= 1e-12 * ev[-1]
    assert abs(rm.value - np.sqrt(lin["cost"] / lin["inliers"])) <= 1e-15
    want = ro.retract(T, -np.linalg.solve(lin["H"], lin["g"]))
    assert np.abs(T1 - want).max() <= 1e-12
    # the states: too few inliers, degenerate, converged -- each leaves the pose alone
    for kw, state in ((dict(min_inliers=10 ** 6), 2), (dict(min_eigenvalue=10.0), 3), (dict(tol_rot=1.0, tol_pos=1.0), 0)):
        q = dict(o)
        q.update(kw)
        T2 = T.copy()
        assert emul.emul_step(got["sums"], q["max_distance"], q["min_inliers"], q["min_eigenvalue"], q["tol_rot"], q["tol_pos"], T2,
                              ctypes.byref(me), ctypes.byref(rm)) == state
        assert np.array_equal(T2, T)


def test_host_jacobi_and_ldlt_against_lapack(emul):
    rng = np.random.default_rng(7)
    for n in (3, 6):
        for cond in (1.0, 1e6):
            B = rng.standard_normal((n, n))
            Q = np.linalg.qr(B)[0]
            lam = np.geomspace(1.0, cond, n)
            A = (Q * lam) @ Q.T
            A = 0.5 * (A + A.T)
            assert abs(emul.emul_jacobi_min(A.copy(), n) - np.linalg.eigvalsh(A)[0]) <= 1e-12 * cond
            b = rng.standard_normal(n)
            x = b.copy()
            assert emul.emul_ldlt_solve(A.copy(), x, n) == 1
            assert np.abs(x - np.linalg.solve(A, b)).max() <= 1e-14 * cond * np.abs(x).max()   # eps x condition number
    sing = np.zeros((6, 6))
    sing[0, 0] = 1.0
    assert emul.emul_ldlt_solve(sing, np.ones(6), 6) == 0 and emul.emul_jacobi_min(sing.copy(), 6) == 0.0


def test_fixture_meets_its_conditions():
    """The conditions the convergence fixture has to meet, on the oracle alone."""
    at = rc.oracle_linearize("truth")
    assert np.sqrt(at["cost"] / at["inliers"]) < 3 * rc.NOISE
    res = rc.oracle_register()
    assert res["status"] == ro.CONVERGED and res["iterations"] <= rc.OPTS["max_iterations"]
    ang, dist = ro.pose_error(res["pose"], rc.truth())
    assert ang <= 1e-3 and dist <= 5e-3
    a0, d0 = ro.pose_error(rc.start(), rc.truth())
    assert ang < a0 and dist < d0
    assert min(t["margin"] for t in res["trace"]) > 1e-9                     # every iteration is comparable across summation orders


def test_struct_sizes_match_the_header():
    L = importlib.import_module("global-lvba_amd._lib")
    # the layout of lvba_register_opts / lvba_register_result against the header: tests/test_abi.py, every struct at once
    assert all(s in L.SYMBOLS for s in ("lvba_register_default_opts", "lvba_register_linearize", "lvba_register_scans"))
