"""The shared pose-graph cases of tests/test_posegraph_host.py and tests/test_gpu_posegraph.py, each relaxed once per process by the
oracle (tests/posegraph_oracle.py).

  pair          N = 2, one closure that contradicts the odometry by a translation, with the odometry's own information: the minimum
                is the midpoint.
  ring64        a ring of 64 poses, every odometry step biased by the same small rotation and translation, closed by one exact
                closure 63 -> 0.  384 unknowns: the builder orders nothing and solves dense.
  ring200       the same with 200 poses: ordered, a narrow band.
  laps130       closure_cases.headed() (three laps of 40) drifted lap by lap, 130 closures lap to lap: a wide coupling.
  two laps      §10e's two laps at the drifted poses with closure_cases.two_lap_closures(extra=False).
  lot320        320 poses, eight stretches of six poses at one place, every stretch tied to every other (tests/test_gpu_nd.py's
                "lot" as closures); lot320 nd is the same under LVBA_SOLVER=nd, which dissects it.
  lever         ring64's closure measured between two lever arms (offsets on both ends).
  cauchy        three mildly drifted laps, twelve true closures and one false one, under CAUCHY.
  anchor 40     ring64 anchored at pose 40.
"""
from __future__ import annotations

import functools

import numpy as np

import band_solve_reference as bsr
import closure_cases as cc
import closure_oracle as co
import posegraph_oracle as pg

STRONG = pg.diag_L(0.002, 0.01)      # a closure's information in the synthetic cases: 5 x the odometry's per step
MARGIN = 1e-6


def ring(N, radius=10.0):
    P = np.zeros((N, 12))
    for k in range(N):
        th = 2.0 * np.pi * k / N
        P[k] = np.r_[(cc.rz(th + 0.5 * np.pi) @ cc.rx(0.02 * np.sin(1.3 * k))).reshape(9), radius * np.cos(th), radius * np.sin(th), 0.1 * np.sin(0.5 * k)]
    return P


def biased(P, rot=(0.0, 0.0, 0.002), trans=(0.01, 0.0, 0.002)):
    """X_0 = P_0, X_{k+1} = X_k (P_k^-1 P_{k+1}) B: every step carries the same bias B"""
    B = co.rigid(rot, trans)
    X = P.copy()
    for k in range(len(P) - 1):
        X[k + 1] = co.mul(X[k], co.mul(co.mul(co.inv(P[k]), P[k + 1]), B))
    return X


def case(name, X, closures, solver=None, env=None, **opts):
    return dict(name=name, X=np.ascontiguousarray(X, np.float64), closures=list(closures), solver=solver, env=env, opts=opts)


def _ring_case(name, N, solver, **opts):
    P = ring(N)
    return case(name, biased(P), [pg.closure(N - 1, 0, co.mul(co.inv(P[N - 1]), P[0]), STRONG)], solver=solver, rel_tol=1e-4, **opts)


def _pair():
    X = ring(8)[:2]
    z = pg.relative(X[0], X[1])
    z[9:] += (0.4, -0.2, 0.1)
    return case("pair", X, [pg.closure(0, 1, z, pg.diag_L(0.01, 0.05))], solver="dense", rel_tol=1e-4)


def _laps130():
    P = cc.headed()
    X = P.copy()
    for f in range(len(P)):   # lap l is turned and moved as a whole: the drift of a lap
        D = co.rigid((0, 0, 0.01 * (f // 40)), (0.3 * (f // 40), -0.2 * (f // 40), 0.0))
        X[f] = co.mul(D, P[f])
    ref, query, Z, _ = cc.grouped(P, 130, lambda k: 0, seed=130)
    return case("laps130", X, [pg.closure(int(i), int(j), z, STRONG) for i, j, z in zip(ref, query, Z)], rel_tol=1e-4)


def two_lap_priors(extra=False, L=STRONG):
    X, ref, query, Z = cc.two_lap_closures(extra=extra)
    return X, [pg.closure(int(i), int(j), z, L) for i, j, z in zip(ref, query, Z)]


def _two_laps():
    X, clo = two_lap_priors()
    return case("two laps", X, clo, rel_tol=1e-4)


WEAK = pg.diag_L(0.02, 0.1)         # the closures of the robust case: a true one starts within the loss scale's reach


def _cauchy():
    """Twelve true closures lap 1 -> laps 2 and 3 of a mildly drifted closure_cases.headed(), and one (the last) whose measurement
    is shifted by 2 m: 20 whitened units against a CAUCHY scale of 3."""
    P = cc.headed()
    X = P.copy()
    for f in range(len(P)):
        X[f] = co.mul(co.rigid((0, 0, 0.004 * (f // 40)), (0.15 * (f // 40), -0.1 * (f // 40), 0.0)), P[f])
    clo = []
    for k in range(12):
        i, j = 3 * k, 3 * k + (40 if k % 2 == 0 else 80)
        clo.append(pg.closure(i, j, co.mul(co.inv(P[i]), P[j]), WEAK))
    z = co.mul(co.inv(P[5]), P[45])
    z[9:] += (2.0, 0.0, 0.0)
    clo.append(pg.closure(5, 45, z, WEAK))
    return case("cauchy", X, clo, rel_tol=1e-4, closure_loss=("cauchy", 3.0))


def _lot(name, env, solver):
    N, Ls = 320, 6
    P = ring(N, radius=40.0)
    starts = [14, 50, 98, 130, 170, 214, 250, 290]
    clo = []
    for a in range(len(starts)):
        for b in range(a + 1, len(starts)):
            for t in range(Ls):
                i, j = starts[a] + t, starts[b] + t
                clo.append(pg.closure(i, j, co.mul(co.inv(P[i]), P[j]), STRONG))
    return case(name, biased(P, rot=(0, 0, 0.0005), trans=(0.003, 0, 0)), clo, solver=solver, env=env, rel_tol=1e-4)


def _lever():
    P = ring(64)
    Oi, Oj = co.rigid((0.1, -0.2, 0.3), (0.5, 0.2, -0.3)), co.rigid((-0.2, 0.1, 0.05), (-0.4, 0.3, 0.6))
    z = co.mul(co.inv(co.mul(P[63], Oi)), co.mul(P[0], Oj))
    return case("lever", biased(P), [pg.closure(63, 0, z, STRONG, oi=Oi, oj=Oj)], rel_tol=1e-4)


@functools.lru_cache(maxsize=None)
def cases():
    return [_pair(), _ring_case("ring64", 64, "dense"), _ring_case("ring200", 200, "band"), _laps130(), _two_laps(),
            _lot("lot320", None, None), _lot("lot320 nd", "nd", "dissected"), _lever(), _cauchy(), _ring_case("anchor 40", 64, "dense", anchor=40)]


def names():
    return [c["name"] for c in cases()]


def named(name):
    return next(c for c in cases() if c["name"] == name)


def graph(c, **more):
    return pg.Graph(c["X"], c["closures"], **dict(c["opts"], **more))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's relaxation of a case (lot320 nd is lot320's graph)"""
    if name == "lot320 nd":
        return oracle("lot320")
    return graph(named(name)).relax()


def band_solve(A, b):
    """the solve as an unpivoted blocked band LDL^T (band_solve_reference) instead of numpy's pivoted LU"""
    L, rcp = bsr.band_ldlt_numpy(A, bsr.bandwidth(A))
    return bsr.band_ldlt_solve(L, rcp, b)


@functools.lru_cache(maxsize=None)
def oracle_band(name):
    return graph(named(name)).relax(solve=band_solve)


def decision_margins(name):
    """(smallest |q| / C1 over the iterations, smallest |q / C1 - rel_tol| / rel_tol over the accepted ones) of the oracle's run"""
    got, tol = oracle(name), pg.options(**named(name)["opts"])["rel_tol"]
    acc = min(r["margin"] for r in got["trace"])
    stop = min(abs(r["q"] / r["residual1"] - tol) / tol for r in got["trace"] if r["accepted"])
    return acc, stop


# Tolerance of the device's poses against the oracle's: both run the same LM in fp64 and differ by the linear solver's rounding.
# Measured on the CPU (tests/test_posegraph_host.py::test_solver_rounding_bound prints and checks it): the largest difference over
# the cases between the oracle with numpy's solve and the oracle with the band LDL^T is 4.6e-13 rad / 3.7e-11 m (lot320, 32
# iterations; every other case is below 1e-15 rad / 1e-14 m); the bound is ten times that.
SOLVER_SPREAD = dict(rot=4.6e-13, pos=3.7e-11)
POSE_TOL = dict(rot=10 * SOLVER_SPREAD["rot"], pos=10 * SOLVER_SPREAD["pos"])
