"""Reference model of the pose-graph relaxation (lvba_posegraph_relax).  TEST INFRASTRUCTURE ONLY: a helper
module, not a test file.

The problem and the LM rule are the header's (include/lvba_hip.h), restated here line by line on top of tests/prior_oracle.py:

    C(x) = sum_i 1/2 |L_o r(X_i, X_{i+1}; Z0_i)|^2 + sum_k 1/2 rho(|L_k r_k(x)|^2) + 1/2 |L_a r_pose(X_a; X0_a)|^2

r / r_pose are prior_oracle's relative / pose residuals, Z0_i = X0_i^-1 X0_{i+1}, rho one of robust_visual_oracle.rho's kinds on
the closures only, with gradient and Gauss-Newton block scaled by rho' and the rho'' term left out.  H is dense, the solve is
numpy.linalg.solve unless another is given (tests/posegraph_cases.py swaps in a band LDL^T to measure the solver's share).
"""
from __future__ import annotations

import numpy as np

import prior_oracle as po
from robust_visual_oracle import rho as loss_rho

DEFAULTS = dict(anchor=0, max_iter=50, odom_sigma_rot=0.01, odom_sigma_pos=0.05, anchor_sigma_rot=1e-4, anchor_sigma_pos=1e-4,
                rel_tol=1e-6, closure_loss=None)
SOLVER_KINDS = {"band": 0, "dissected": 1, "dense": 2}


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    return o


def relative(Xi, Xj):
    """X_i^-1 X_j as 12 numbers"""
    Ri, pi = po._Rp(Xi)
    Rj, pj = po._Rp(Xj)
    return np.r_[(Ri.T @ Rj).reshape(9), Ri.T @ (pj - pi)]


def diag_L(sr, sp):
    return np.diag([1.0 / sr] * 3 + [1.0 / sp] * 3)


def odometry_edges(X0, sigma_rot, sigma_pos):
    X0 = np.asarray(X0, np.float64).reshape(-1, 12)
    L = diag_L(sigma_rot, sigma_pos)
    return [po.make_prior("relative", i, relative(X0[i], X0[i + 1]), L, j=i + 1) for i in range(len(X0) - 1)]


def closure(i, j, meas, L, oi=None, oj=None):
    return po.make_prior("relative", i, meas, L, j=j, oi=oi, oj=oj)


def _loss(loss, s):
    if loss is None or loss[0] == "trivial":
        return s, 1.0
    r = loss_rho(loss[0], loss[1], s)
    return r[0], r[1]


class Graph:
    def __init__(self, X0, closures, **opts):
        self.o = options(**opts)
        self.X0 = np.array(X0, np.float64).reshape(-1, 12)
        self.N = len(self.X0)
        self.odo = odometry_edges(self.X0, self.o["odom_sigma_rot"], self.o["odom_sigma_pos"])
        self.clo = list(closures)
        a = self.o["anchor"]
        self.anc = po.make_prior("pose", a, self.X0[a], diag_L(self.o["anchor_sigma_rot"], self.o["anchor_sigma_pos"]))

    def edges(self):
        """(prior, class) in the library's order: odometry, closures, anchor"""
        return [(p, 0) for p in self.odo] + [(p, 1) for p in self.clo] + [(self.anc, 2)]

    def edge(self, pr, cls, x, jac=True):
        """(cost, weight, e, Wi, Wj) of one edge: e and W un-weighted"""
        r, Ji, Jj = po.raw(pr, x[pr["i"]], x[pr["j"]] if pr["kind"] == 2 else None)
        e, Wi, Wj = po.whiten(pr, r, Ji, Jj)
        s = float(e @ e)
        rho, w = _loss(self.o["closure_loss"], s) if cls == 1 else (s, 1.0)
        return 0.5 * rho, w, e, Wi, Wj

    def costs(self, x):
        """(C, odometry sum, closure sum, closure weights)"""
        x = np.asarray(x, np.float64).reshape(-1, 12)
        c = [0.0, 0.0, 0.0]
        w = []
        for pr, cls in self.edges():
            ck, wk, _, _, _ = self.edge(pr, cls, x)
            c[cls] += ck
            if cls == 1:
                w.append(wk)
        return c[0] + c[1] + c[2], c[0], c[1], np.array(w)

    def cost(self, x):
        return self.costs(x)[0]

    def assemble(self, x):
        """(H [6N, 6N], g [6N], C) in the caller's pose order"""
        x = np.asarray(x, np.float64).reshape(-1, 12)
        n = 6 * self.N
        H, g, c = np.zeros((n, n)), np.zeros(n), 0.0
        for pr, cls in self.edges():
            ck, w, e, Wi, Wj = self.edge(pr, cls, x)
            c += ck
            si = slice(6 * pr["i"], 6 * pr["i"] + 6)
            H[si, si] += w * (Wi.T @ Wi)
            g[si] += w * (Wi.T @ e)
            if pr["kind"] == 2:
                sj = slice(6 * pr["j"], 6 * pr["j"] + 6)
                H[sj, sj] += w * (Wj.T @ Wj)
                H[si, sj] += w * (Wi.T @ Wj)
                H[sj, si] += w * (Wj.T @ Wi)
                g[sj] += w * (Wj.T @ e)
        return H, g, c

    def relax(self, solve=np.linalg.solve, max_iter=None, rel_tol=None):
        """The header's LM rule.  Returns dict(poses, weights, trace, report); every trace row also holds `margin`, the relative
        distance of its accept decision from its threshold, |q| / C1."""
        max_iter = self.o["max_iter"] if max_iter is None else max_iter
        rel_tol = self.o["rel_tol"] if rel_tol is None else rel_tol
        x = self.X0.copy()
        trace = []
        rep = dict(iterations=0, accepted=0, status=0, cost_first=0.0, max_step_last=0.0)
        if not self.clo:
            rep.update(cost_last=0.0, odom_cost_last=0.0, closure_cost_last=0.0)
            return dict(poses=x, weights=np.zeros(0), trace=trace, report=rep)
        u, v = 0.01, 2.0
        H = g = None
        C1 = 0.0
        evaluate = True
        for it in range(max_iter):
            evaluated = evaluate
            if evaluate:
                H, g, C1 = self.assemble(x)
                if it == 0:
                    rep["cost_first"] = C1
                    if C1 == 0.0:
                        break
            D = np.diag(H).copy()
            dx = solve(H + u * np.diag(D), -g)
            x2 = po.retract(x, dx)
            q1 = 0.5 * float(dx @ (u * D * dx - g))
            C2 = self.cost(x2)
            q = C1 - C2
            trace.append(dict(iter=it, accepted=int(q > 0), evaluated=int(evaluated), status=0, residual1=C1, residual2=C2, u=u, v=v, q=q,
                              q1=q1, margin=abs(q) / C1))
            rep["iterations"] += 1
            stop = False
            if q > 0:
                x = x2
                rep["accepted"] += 1
                rep["max_step_last"] = float(np.abs(dx).max())
                t = 1.0 - (2.0 * (q / q1) - 1.0) ** 3
                u *= 1.0 / 3.0 if t < 1.0 / 3.0 else t
                v = 2.0
                evaluate = True
                stop = q / C1 < rel_tol
            else:
                u *= v
                v *= 2.0
                evaluate = False
            if stop:
                break
        if max_iter == 0:
            rep["cost_first"] = self.cost(x)
        c = self.costs(x)
        rep.update(cost_last=c[0], odom_cost_last=c[1], closure_cost_last=c[2])
        return dict(poses=x, weights=c[3], trace=trace, report=rep)


def pose_errors(A, B):
    """(largest rotation angle [rad], largest position distance [m]) between two pose arrays"""
    A, B = np.asarray(A, np.float64).reshape(-1, 12), np.asarray(B, np.float64).reshape(-1, 12)
    rot = max(float(np.linalg.norm(po.so3_log(a[:9].reshape(3, 3).T @ b[:9].reshape(3, 3)))) for a, b in zip(A, B))
    return rot, float(np.linalg.norm(A[:, 9:] - B[:, 9:], axis=1).max())
