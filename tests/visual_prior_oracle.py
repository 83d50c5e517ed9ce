"""Reference model of the visual stage's camera pose priors (lvba_visual_set_priors).  TEST INFRASTRUCTURE ONLY: a helper module,
not a test file.

A camera k is (q_k, t_k) = T_cam<-world (q = [w,x,y,z], normalised before it rotates, as ceres::QuaternionRotatePoint does); the
pose a prior sees is T_k = T_world<-cam = (R^T, -R^T t).  With A = T_i O_i, B = T_j O_j (offsets O = (R_O, p_O), identity when
twelve zeros):
    POSE      r = [Log(Rm^T R_A); p_A - pm]
    POSITION  r = p_A - z                                   (3 rows, the top-left 3 x 3 of sqrt_info; e[3..5] = 0)
    RELATIVE  r = [Log(Rm^T R_A^T R_B); R_A^T (p_B - p_A) - pm]
e = L r, cost 1/2 |e|^2, never under a loss.  The three residuals are written here in torch from these formulas, differentiated
by autograd w.r.t. the ambient (q, t) and projected onto the visual tangent with EigenQuaternionManifold::PlusJacobian
(oracle.visual_oracle.eigen_quat_plus_jacobian) -- nothing of csrc/prior_device.h is restated.

VisualPriorOracle appends these rows (6 per prior, after the Corrector has been applied to the reprojection / plane blocks) to
what RobustVisualOracle returns, so the parent's solve, reduced_system and gradient_max_norm see them as one more residual block
each.  Without priors it performs the parent's arithmetic bit for bit.  Priors are `lvba_prior` structs (balm.Prior.*).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.visual_oracle import eigen_quat_plus_jacobian
from robust_visual_oracle import RobustVisualOracle

F64 = torch.float64
POSE, POSITION, RELATIVE = 0, 1, 2


def _rot(q):
    """R(q / |q|) for q = [w,x,y,z]."""
    w, x, y, z = q / q.norm()
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])


def _log(R):
    """Log of SO(3): theta = atan2(|w|, (tr - 1) / 2), w = vee(R - R^T) / 2, phi = theta / |w| * w (a polynomial at |w| -> 0)."""
    w = 0.5 * torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    s2 = w @ w
    if float(s2.detach()) < 1e-16 and float(c.detach()) > 0.0:
        return w * (1.0 + s2 / 6.0)
    s = torch.sqrt(s2)
    return torch.atan2(s, c) / s * w


def world_pose(q, t):
    """T_world<-cam = (R^T, -R^T t)."""
    Rt = _rot(q).T
    return Rt, -(Rt @ t)


def _offset(o):
    o = np.asarray(o, np.float64)
    if not o.any():
        return torch.eye(3, dtype=F64), torch.zeros(3, dtype=F64)
    return torch.tensor(o[:9].reshape(3, 3), dtype=F64), torch.tensor(o[9:], dtype=F64)


def prior_fields(p):
    """(kind, i, j, meas [12], offset_i [12], offset_j [12], L [6, 6]) of an lvba_prior struct."""
    return (int(p.kind), int(p.i), int(p.j), np.array(list(p.meas)), np.array(list(p.offset_i)), np.array(list(p.offset_j)),
            np.array(list(p.sqrt_info)).reshape(6, 6))


def whitened_residual(p, qi, ti, qj, tj):
    """e [6] (torch) of one prior at the cameras (qi, ti), (qj, tj): torch tensors, differentiable."""
    kind, _i, _j, meas, oi, oj, L = prior_fields(p)
    Rm, pm = torch.tensor(meas[:9].reshape(3, 3), dtype=F64), torch.tensor(meas[9:], dtype=F64)
    Ri, pi = world_pose(qi, ti)
    ROi, pOi = _offset(oi)
    RA, pA = Ri @ ROi, Ri @ pOi + pi
    if kind == POSITION:
        e3 = torch.tensor(L[:3, :3], dtype=F64) @ (pA - pm)
        return torch.cat([e3, torch.zeros(3, dtype=F64)])
    if kind == POSE:
        r = torch.cat([_log(Rm.T @ RA), pA - pm])
    else:
        Rj, pj = world_pose(qj, tj)
        ROj, pOj = _offset(oj)
        RB, pB = Rj @ ROj, Rj @ pOj + pj
        r = torch.cat([_log(Rm.T @ RA.T @ RB), RA.T @ (pB - pA) - pm])
    return torch.tensor(L, dtype=F64) @ r


def prior_block(p, q, t, want_jac=True):
    """(e [6], Wi [6, 6], Wj [6, 6]) of one prior at the camera arrays q [M, 4], t [M, 3]: the whitened residual and its Jacobians
    in the visual tangents [dq(3), dt(3)] of cameras i and j (Wj zero unless RELATIVE)."""
    kind, i, j = int(p.kind), int(p.i), int(p.j)
    if kind != RELATIVE:
        j = i
    qi = torch.tensor(q[i], dtype=F64, requires_grad=want_jac)
    ti = torch.tensor(t[i], dtype=F64, requires_grad=want_jac)
    qj = torch.tensor(q[j], dtype=F64, requires_grad=want_jac)
    tj = torch.tensor(t[j], dtype=F64, requires_grad=want_jac)
    e = whitened_residual(p, qi, ti, qj, tj)
    Wi, Wj = np.zeros((6, 6)), np.zeros((6, 6))
    if want_jac:
        Pi, Pj = eigen_quat_plus_jacobian(q[i]), eigen_quat_plus_jacobian(q[j])
        for a in range(6):
            if not e[a].requires_grad:
                continue
            g = torch.autograd.grad(e[a], (qi, ti, qj, tj), retain_graph=True, allow_unused=True)
            g = [np.zeros(n) if v is None else v.numpy() for v, n in zip(g, (4, 3, 4, 3))]
            Wi[a, :3], Wi[a, 3:] = g[0] @ Pi, g[1]
            if kind == RELATIVE:
                Wj[a, :3], Wj[a, 3:] = g[2] @ Pj, g[3]
    return e.detach().numpy(), Wi, Wj


class VisualPriorOracle(RobustVisualOracle):
    """RobustVisualOracle + camera pose priors: a list of lvba_prior structs with caller camera indices."""

    def __init__(self, p, priors=(), reproj=None, plane=None):
        super().__init__(p, reproj, plane)
        self.priors = list(priors or [])

    def prior_residuals(self, q, t):
        """(e [n, 6], cost)"""
        e = np.array([prior_block(p, q, t, False)[0] for p in self.priors]).reshape(-1, 6)
        return e, 0.5 * float((e * e).sum())

    def prior_rows(self, q, t, want_jac=True):
        """(e [6 n], J [6 n, n_par] or None): camera 0 is constant, its columns do not exist."""
        es, Js = [], []
        for p in self.priors:
            e, Wi, Wj = prior_block(p, q, t, want_jac)
            es.append(e)
            if want_jac:
                J = np.zeros((6, self.n_par))
                for c, W in ((int(p.i), Wi), (int(p.j), Wj)):
                    if c > 0 and (W is Wi or int(p.kind) == RELATIVE):
                        J[:, 6 * (c - 1):6 * c] = W
                Js.append(J)
        return np.concatenate(es), (np.concatenate(Js, 0) if want_jac else None)

    def residuals_and_jacobian(self, q, t, X, want_jac=True):
        rt, Jt, s, rho0 = super().residuals_and_jacobian(q, t, X, want_jac)
        if not self.priors:
            return rt, Jt, s, rho0
        e, Je = self.prior_rows(q, t, want_jac)
        sk = (e.reshape(-1, 6) ** 2).sum(1)                   # a prior block's rho(s) = s: the trivial loss
        return (np.concatenate([rt, e]), np.concatenate([Jt, Je], 0) if want_jac else None, np.concatenate([s, sk]),
                np.concatenate([rho0, sk]))
