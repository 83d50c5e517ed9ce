"""Reference model of the visual stage's robust losses (lvba_visual_set_loss).  TEST INFRASTRUCTURE ONLY: a helper module, not a
test file.

Loss functions: Ceres Solver 2.1.0's HuberLoss, SoftLOneLoss, CauchyLoss, ArctanLoss and TukeyLoss (internal/ceres/loss_function.cc),
restated from its published sources in plain Python floats with the C library's math functions (the device header
csrc/visual_loss.h is held to these within a few ulp by tests/test_visual_loss_host.py).  Ceres' Corrector
(internal/ceres/corrector.cc) for rho'' <= 0: r~ = sqrt(rho') r, J~ = sqrt(rho') J; a block contributes 1/2 rho(s) to the cost.

RobustVisualOracle restates oracle.visual_oracle.VisualOracle.solve (its Ceres 2.1 trust-region loop) with those three
changes: the linearisation is (r~, J~), and both the cost at the linearisation point and the cost of a trial point are
1/2 sum rho(s).  With both families TRIVIAL it performs exactly the parent's arithmetic.
"""
from __future__ import annotations

import math
import sys

import numpy as np

from oracle.visual_oracle import VisualOracle, eigen_quat_plus  # noqa: F401  (eigen_quat_plus: re-exported for the tests)

KINDS = {"trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}
DBL_MIN = sys.float_info.min


def rho(kind, a, s):
    """(rho, rho', rho'') of one block with squared norm s >= 0; kind a KINDS name, a the scale."""
    s = float(s)
    if kind == "trivial":
        return s, 1.0, 0.0
    a = float(a)
    b = a * a
    if kind == "huber":
        if s > b:
            r = math.sqrt(s)
            d1 = max(DBL_MIN, a / r)
            return 2.0 * a * r - b, d1, -d1 / (2.0 * s)
        return s, 1.0, 0.0
    c = 1.0 / b
    if kind == "softlone":
        total = 1.0 + s * c
        tmp = math.sqrt(total)
        d1 = max(DBL_MIN, 1.0 / tmp)
        return 2.0 * b * (tmp - 1.0), d1, -(c * d1) / (2.0 * total)
    if kind == "cauchy":
        total = 1.0 + s * c
        inv = 1.0 / total
        return b * math.log(total), max(DBL_MIN, inv), -c * (inv * inv)
    if kind == "arctan":
        total = 1.0 + s * s * c
        inv = 1.0 / total
        return a * math.atan2(s, a), max(DBL_MIN, inv), -2.0 * s * c * (inv * inv)
    if kind == "tukey":
        if s <= b:
            v = 1.0 - s / b
            v2 = v * v
            return b / 3.0 * (1.0 - v2 * v), v2, -2.0 / b * v
        return b / 3.0, 0.0, 0.0
    raise ValueError(kind)


def rho_vec(kind, a, s):
    """rho() over an array: [n, 3]."""
    return np.array([rho(kind, a, v) for v in np.asarray(s, np.float64).reshape(-1)]).reshape(-1, 3)


def _norm_loss(loss):
    if loss is None:
        return ("trivial", 0.0)
    kind, a = loss
    kind = str(kind).lower()
    if kind not in KINDS:
        raise ValueError(kind)
    return (kind, float(a))


def add_outliers(d, frac, seed, lo=20.0, hi=100.0):
    """A copy of the synthetic problem d with a share `frac` of its observations displaced by lo..hi pixels in a random direction
    (a generator of its own: synth's output is untouched).  Returns (d2, mask of the displaced observations)."""
    rng = np.random.default_rng(seed)
    d2 = dict(d)
    uv = d["obs_uv"].copy()
    n = len(uv)
    idx = rng.choice(n, size=int(round(frac * n)), replace=False)
    ang = rng.uniform(0.0, 2.0 * np.pi, len(idx))
    mag = rng.uniform(lo, hi, len(idx))
    uv[idx, 0] += mag * np.cos(ang)
    uv[idx, 1] += mag * np.sin(ang)
    d2["obs_uv"] = uv
    mask = np.zeros(n, bool)
    mask[idx] = True
    return d2, mask


class RobustVisualOracle(VisualOracle):
    """VisualOracle with a loss on the reprojection blocks (one 2-vector per observation) and one on the plane blocks (one per
    active landmark): None or (kind, a)."""

    def __init__(self, p, reproj=None, plane=None):
        super().__init__(p)
        self.loss = (_norm_loss(reproj), _norm_loss(plane))
        self.trivial = self.loss[0][0] == "trivial" and self.loss[1][0] == "trivial"
        blk, fam = [], []
        for b, (kind, _li, _ti, _o) in enumerate(self.rows):
            blk += [b] * (2 if kind == "r" else 1)
            fam.append(0 if kind == "r" else 1)
        self.row_block = np.asarray(blk, np.int64)
        self.block_family = np.asarray(fam, np.int64)

    def block_sq(self, r):
        """s per residual block (row order of self.rows) from the stacked residual vector."""
        s = np.zeros(len(self.rows))
        k = 0
        for b, (kind, _li, _ti, _o) in enumerate(self.rows):
            if kind == "r":
                s[b] = r[k] * r[k] + r[k + 1] * r[k + 1]
                k += 2
            else:
                s[b] = r[k] * r[k]
                k += 1
        return s

    def block_rho(self, s):
        out = np.empty((len(s), 3))
        for f in (0, 1):
            sel = self.block_family == f
            kind, a = self.loss[f]
            out[sel] = rho_vec(kind, a, s[sel]) if sel.any() else np.zeros((0, 3))
        return out

    def residuals_and_jacobian(self, q, t, X, want_jac=True):
        """(r~, J~, s, rho): the Corrector applied to the parent's residuals and Jacobian, plus per block s and rho(s)."""
        r, J = super().residuals_and_jacobian(q, t, X, want_jac)
        return self.correct(r, J)

    def correct(self, r, J):
        """The Corrector on the parent's (r, J) (J may be None): (r~, J~, s, rho) -- the losses of this oracle, the residuals of
        any VisualOracle of the same problem."""
        s = self.block_sq(r)
        rh = self.block_rho(s)
        w = np.sqrt(rh[:, 1])[self.row_block]
        rt = r * w
        Jt = J * w[:, None] if J is not None else None
        return rt, Jt, s, rh[:, 0]

    def _cost(self, rt, rho0):
        if self.trivial:                     # the parent's arithmetic, bit for bit
            return 0.5 * float(rt @ rt)
        return 0.5 * float(rho0.sum())

    def cost(self, q, t, X):
        rt, _, _, rho0 = self.residuals_and_jacobian(q, t, X, want_jac=False)
        return self._cost(rt, rho0)

    def linearization(self, q, t, X, radius):
        """Dense reduced camera system of the corrected Jacobian with its own Jacobi scaling (what lvba_visual_linearize
        exports): (S, rhs, cost) over cameras 1..M-1."""
        return self.reduced_system(*self.residuals_and_jacobian(q, t, X), radius)

    def reduced_system(self, r, J, _s, rho0, radius):
        """(S, rhs, cost) from the corrected (r~, J~, s, rho) of correct()."""
        scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
        J = J * scale
        D2 = np.clip((J * J).sum(0), 1e-6, 1e32) / radius
        A = J.T @ J + np.diag(D2)
        g = J.T @ r
        nc = self.n_cam
        B, E, Cm = A[:nc, :nc], A[:nc, nc:], A[nc:, nc:]
        Ci = np.zeros_like(Cm)
        for i in range(len(self.act)):
            sl = slice(3 * i, 3 * i + 3)
            Ci[sl, sl] = np.linalg.inv(Cm[sl, sl])
        return B - E @ Ci @ E.T, g[:nc] - E @ (Ci @ g[nc:]), self._cost(r, rho0)

    # VisualOracle.solve with 1/2 sum rho(s) where it has 1/2 r.r ---------------------------------------------------------
    def solve(self, max_iter=50, verbose=False):
        q, t, X = self.state()
        radius, decrease_factor = 1e4, 2.0
        min_diag, max_diag = 1e-6, 1e32
        r, J, _s, rho0 = self.residuals_and_jacobian(q, t, X)
        cost = self._cost(r, rho0)
        scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
        J = J * scale
        trace = [dict(iter=0, cost=cost, cost_change=0.0, step_norm=0.0, radius=radius, accepted=1, rho=0.0)]
        status = "NO_CONVERGENCE"
        g = J.T @ r
        if max_iter <= 0:
            return (q, t, X), trace, "NO_CONVERGENCE"
        if self.gradient_max_norm(q, g / scale) <= 1e-10:
            return (q, t, X), trace, "CONVERGENCE(gradient)"
        invalid_run = 0
        x_norm = float(np.sqrt((q[1:] ** 2).sum() + (t[1:] ** 2).sum() + (X[self.act] ** 2).sum()))
        it = 0
        while True:
            it += 1
            if it > max_iter:
                break
            diag = np.clip((J * J).sum(0), min_diag, max_diag)
            D = np.sqrt(diag / radius)
            x = self.solve_schur(J, r, D)
            step = -x
            mr = J @ step if np.all(np.isfinite(step)) else None
            model_cost_change = -float(mr @ (r + mr / 2.0)) if mr is not None else 0.0
            if mr is None or model_cost_change <= 0.0:
                radius = radius / decrease_factor
                decrease_factor *= 2.0
                trace.append(dict(iter=it, cost=cost, cost_change=0.0, step_norm=0.0, radius=radius, accepted=0, rho=0.0))
                invalid_run += 1
                if invalid_run >= 5:
                    status = "FAILURE"
                    break
                if radius < 1e-32:
                    status = "CONVERGENCE(radius)"
                    break
                continue
            invalid_run = 0
            delta = step * scale
            q2, t2, X2 = self.plus(q, t, X, delta)
            cand = self.cost(q2, t2, X2)
            step_norm = float(np.sqrt(((q2 - q) ** 2).sum() + ((t2 - t) ** 2).sum() + ((X2 - X) ** 2).sum()))
            if step_norm <= 1e-8 * (x_norm + 1e-8):
                trace.append(dict(iter=it, cost=cost, cost_change=cost - cand, step_norm=step_norm, radius=radius, accepted=0, rho=0.0))
                status = "CONVERGENCE(parameter)"
                break
            cost_change = cost - cand
            if abs(cost_change) <= 1e-6 * cost:
                trace.append(dict(iter=it, cost=cost, cost_change=cost_change, step_norm=step_norm, radius=radius, accepted=0, rho=0.0))
                status = "CONVERGENCE(function)"
                break
            rho_step = cost_change / model_cost_change
            if rho_step > 1e-3:
                q, t, X = q2, t2, X2
                x_norm = float(np.sqrt((q[1:] ** 2).sum() + (t[1:] ** 2).sum() + (X[self.act] ** 2).sum()))
                r, J, _s, rho0 = self.residuals_and_jacobian(q, t, X)
                J = J * scale
                cost = self._cost(r, rho0)
                radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho_step - 1.0) ** 3))
                decrease_factor = 2.0
                trace.append(dict(iter=it, cost=cost, cost_change=cost_change, step_norm=step_norm, radius=radius, accepted=1,
                                  rho=rho_step))
                g = J.T @ r
                if it >= max_iter:
                    break
                if self.gradient_max_norm(q, g / scale) <= 1e-10:
                    status = "CONVERGENCE(gradient)"
                    break
            else:
                radius = radius / decrease_factor
                decrease_factor *= 2.0
                trace.append(dict(iter=it, cost=cand, cost_change=cost_change, step_norm=step_norm, radius=radius, accepted=0,
                                  rho=rho_step))
                if radius < 1e-32:
                    status = "CONVERGENCE(radius)"
                    break
            if verbose:
                print(trace[-1])
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        return (q, t, X), trace, status
