"""Reference model of the LiDAR stage's pose priors (lvba_balm_set_priors).  TEST INFRASTRUCTURE ONLY: a helper module, not a
test file.

A pose is T = (R, p), 12 doubles R row-major | p; the update is R <- R Exp(phi), p <- p + dp (bavoxel.hpp:722-727).  A prior is a
dict(kind, i, j, meas [12], oi [12], oj [12], L [6, 6]); with A = T_i O_i and B = T_j O_j its residual is
    pose      [Log(Rm^T R_A); p_A - pm]
    position  p_A - z               (z = meas[9:12], 3 rows, L[:3, :3])
    relative  [Log(Rm^T R_A^T R_B); R_A^T (p_B - p_A) - pm]
and it adds 1/2 |L r|^2 to the cost, J^T L^T L r to g and J^T L^T L J to H (Gauss-Newton).  The formulas follow
csrc/prior_device.h step by step (same Log, Exp and Jr^-1 branches), so the two agree to a few ulp; the Jacobians are pinned
independently by central finite differences (tests/test_priors_host.py).

PriorOracle.damping_iter restates oracle.balm_oracle.damping_iter with H += J^T J, g += J^T e and the prior cost added to both
costs, averaged over the voxel count like the voxel sum.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import balm_oracle as bo

KINDS = {"pose": 0, "position": 1, "relative": 2}
IDENT = np.r_[np.eye(3).reshape(-1), 0.0, 0.0, 0.0]


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_log(R):
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    s = math.sqrt(w @ w)
    th = math.atan2(s, c)
    if c > -0.9:
        if th < 1e-4:
            t2 = th * th
            f = 1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0
        else:
            f = th / s
        return f * w
    S = np.diag(R) - c
    k = 0
    if S[1] > S[0] and S[1] >= S[2]:
        k = 1
    elif S[2] > S[0] and S[2] > S[1]:
        k = 2
    a = 0.5 * (R[:, k] + R[k, :])
    a[k] = S[k]
    n = math.sqrt(a @ a)
    if a @ w < 0.0:
        n = -n
    return (th / n) * a


def so3_exp(w):
    return bo.exp_so3(w)


def jr_inv(p):
    p = np.asarray(p, np.float64)
    t2 = float(p @ p)
    th = math.sqrt(t2)
    if th < 1e-2:
        b = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0
    else:
        b = 1.0 / t2 - math.cos(0.5 * th) / (2.0 * th * math.sin(0.5 * th))
    K = hat(p)
    return np.eye(3) + 0.5 * K + b * (K @ K)


def _Rp(T):
    T = np.asarray(T, np.float64).reshape(12)
    return T[:9].reshape(3, 3), T[9:12]


def compose(T, O):
    R, p = _Rp(T)
    Ro, po = _Rp(O)
    return R @ Ro, R @ po + p


def raw(pr, Ti, Tj=None):
    """(r [6], Ji [6, 6], Jj [6, 6]) of the un-whitened residual (position: rows 3..5 zero)."""
    kind = pr["kind"]
    Rm, pm = _Rp(pr["meas"])
    Ri, _ = _Rp(Ti)
    Roi, poi = _Rp(pr["oi"])
    RA, pA = compose(Ti, pr["oi"])
    r = np.zeros(6)
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    if kind == 1:
        r[:3] = pA - pm
        Ji[:3, :3] = -Ri @ hat(poi)
        Ji[:3, 3:] = np.eye(3)
        return r, Ji, Jj
    if kind == 0:
        r[:3] = so3_log(Rm.T @ RA)
        r[3:] = pA - pm
        Ji[:3, :3] = jr_inv(r[:3]) @ Roi.T
        Ji[3:, :3] = -Ri @ hat(poi)
        Ji[3:, 3:] = np.eye(3)
        return r, Ji, Jj
    Rj, _ = _Rp(Tj)
    Roj, poj = _Rp(pr["oj"])
    RB, pB = compose(Tj, pr["oj"])
    M = RA.T @ RB
    r[:3] = so3_log(Rm.T @ M)
    q = RA.T @ (pB - pA)
    r[3:] = q - pm
    Jr = jr_inv(r[:3])
    Ji[:3, :3] = -Jr @ M.T @ Roi.T
    Ji[3:, :3] = hat(q) @ Roi.T + Roi.T @ hat(poi)
    Ji[3:, 3:] = -RA.T
    Jj[:3, :3] = Jr @ Roj.T
    Jj[3:, :3] = -RA.T @ Rj @ hat(poj)
    Jj[3:, 3:] = RA.T
    return r, Ji, Jj


def whiten(pr, r, Ji, Jj):
    m = 3 if pr["kind"] == 1 else 6
    L = np.zeros((6, 6))
    L[:m, :m] = np.asarray(pr["L"], np.float64).reshape(6, 6)[:m, :m]
    return L @ r, L @ Ji, L @ Jj


def residual(pr, poses):
    """whitened e [6] and the prior's cost 1/2 |e|^2 at poses [N, 12]"""
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    r, _, _ = raw(pr, x[pr["i"]], x[pr["j"]] if pr["kind"] == 2 else None)
    e, _, _ = whiten(pr, r, np.zeros((6, 6)), np.zeros((6, 6)))
    return e, 0.5 * float(e @ e)


def assemble(priors, poses):
    """(H [6N, 6N], g [6N], cost) of the priors alone (caller's pose order)."""
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    n = 6 * x.shape[0]
    H, g, c = np.zeros((n, n)), np.zeros(n), 0.0
    for pr in priors:
        i = pr["i"]
        r, Ji, Jj = raw(pr, x[i], x[pr["j"]] if pr["kind"] == 2 else None)
        e, Wi, Wj = whiten(pr, r, Ji, Jj)
        c += 0.5 * float(e @ e)
        si = slice(6 * i, 6 * i + 6)
        H[si, si] += Wi.T @ Wi
        g[si] += Wi.T @ e
        if pr["kind"] == 2:
            j = pr["j"]
            sj = slice(6 * j, 6 * j + 6)
            H[sj, sj] += Wj.T @ Wj
            H[si, sj] += Wi.T @ Wj
            H[sj, si] += Wj.T @ Wi
            g[sj] += Wj.T @ e
    return H, g, c


def retract(poses, dx):
    return bo.retract(poses, dx)


def make_prior(kind, i, meas, L, j=0, oi=None, oj=None):
    return dict(kind=KINDS[kind] if isinstance(kind, str) else int(kind), i=int(i), j=int(j),
                meas=np.asarray(meas, np.float64).reshape(12), oi=IDENT.copy() if oi is None else np.asarray(oi, np.float64).reshape(12),
                oj=IDENT.copy() if oj is None else np.asarray(oj, np.float64).reshape(12), L=np.asarray(L, np.float64).reshape(6, 6))


class PriorOracle:
    """A BALM problem (oracle.COracle) plus priors."""

    def __init__(self, co, priors):
        self.co, self.priors = co, list(priors)

    def eval_dense(self, poses):
        """(H, g, cost) summed over voxels and priors (COracle.eval_dense averages its cost over the voxels)"""
        H, g, c = self.co.eval_dense(poses)
        Hp, gp, cp = assemble(self.priors, poses)
        return H + Hp, g + gp, c * self.co.V + cp

    def cost(self, poses):
        return self.co.cost(poses) + assemble(self.priors, poses)[2]

    def damping_iter(self, poses, max_iter=10, u0=0.01, v0=2.0, rel_tol=1e-6):
        """oracle.balm_oracle.damping_iter (bavoxel.hpp:662-767) with the priors in H, g and both costs."""
        V = self.co.V

        def ev(x):
            H, g, c = self.eval_dense(x)
            return H, g, c / V

        import oracle  # the C oracle's unpivoted dense LDL^T: the factorisation the GPU solvers perform

        def solve(A, b):
            x, rc = oracle.ldlt_solve_dense(A, b)
            assert rc == 0
            return x

        x, trace = bo.damping_iter(_V(V), poses, max_iter, u0, v0, rel_tol, eval_fn=ev, cost_fn=lambda x: self.cost(x) / V,
                                   solve_fn=solve)
        return x, trace


class _V:
    def __init__(self, V):
        self.n_voxels = V
