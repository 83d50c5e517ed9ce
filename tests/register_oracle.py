"""CPU restatement of the scan-to-map registration (lvba_register_linearize / lvba_register_scans, csrc/register_device.h) on
top of oracle.voxel_oracle.build / find_plane.  TEST INFRASTRUCTURE ONLY.

One job = one cloud P [m, 3] (fp32, promoted once) and a pose T = (R row-major | t).  Per point
    w   = (R00 px + R01 py) + R02 pz + tx, ...          (this operation order, elementwise)
    (n, d) = find_plane(w)                               (the landmark -> plane lookup of the voxel front-end)
    r   = (n0 w0 + n1 w1) + n2 w2 + d
    inlier iff a plane was found and |r| <= max_distance
    J   = [ p x (R^T n) ; n ]                            (d r / d(theta, t) under R <- R Exp(theta), t <- t + delta)
    s = r^2, (rho, rho') = loss(s):  H += rho' J J^T, g += rho' J r, cost += rho          (no loss: rho = s, rho' = 1)
and per iteration
    too few inliers (< min_inliers)  |  degenerate (smallest eigenvalue of H / inliers < min_eigenvalue)  |
    delta = -H^-1 g;  converged (|dtheta| <= tol_rot and |dt| <= tol_pos: the step is NOT applied)  |  retract and continue.
`information` is H of the last linearisation, rmse = sqrt(cost_last / inliers).

Every linearisation also reports the smallest DECISION MARGIN: the distance of any |r| to max_distance and of any world
coordinate to a multiple of voxel_size / 4 (every root and octant face is one).  A result computed in another summation order can
only take another discrete decision where that margin is of the order of its rounding error.
"""
from __future__ import annotations

import numpy as np

from oracle import voxel_oracle as vo
from robust_visual_oracle import rho_vec

CONVERGED, MAX_ITERATIONS, TOO_FEW_INLIERS, DEGENERATE = 0, 1, 2, 3
TRI = [(a, b) for a in range(6) for b in range(a, 6)]                      # the 21 upper-triangle entries, row-major


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    """Rodrigues (prior_device.h: so3_exp)."""
    w = np.asarray(w, np.float64)
    t2 = float(w @ w)
    th = np.sqrt(t2)
    if th < 1e-4:
        A, B = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        A, B = np.sin(th) / th, 2.0 * (np.sin(0.5 * th) / th) ** 2
    K = hat(w)
    return np.eye(3) + A * K + B * (K @ K)


def retract(T, dx):
    T = np.asarray(T, np.float64).reshape(12)
    R = T[:9].reshape(3, 3) @ exp_so3(dx[:3])
    return np.r_[R.reshape(9), T[9:] + dx[3:]]


def world_points(T, P):
    T = np.asarray(T, np.float64).reshape(12)
    P = np.asarray(P, np.float32).astype(np.float64)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([(T[3 * k] * px + T[3 * k + 1] * py) + T[3 * k + 2] * pz + T[9 + k] for k in range(3)], 1)


def associate(surf, vs, W):
    """(plane [m, 4], found [m]) of world points W."""
    plane, found = np.zeros((len(W), 4)), np.zeros(len(W), bool)
    for i, w in enumerate(W):
        pl = vo.find_plane(surf, w, vs) if surf else None
        if pl is not None:
            plane[i, :3], plane[i, 3], found[i] = pl[0], pl[1], True
    return plane, found


def residuals(T, P, plane):
    """r [m] and J [m, 6] for given planes (the smooth part: the association is held fixed)."""
    T = np.asarray(T, np.float64).reshape(12)
    W = world_points(T, P)
    P64 = np.asarray(P, np.float32).astype(np.float64)
    n = plane[:, :3]
    r = (n[:, 0] * W[:, 0] + n[:, 1] * W[:, 1]) + n[:, 2] * W[:, 2] + plane[:, 3]
    R = T[:9].reshape(3, 3)
    u = np.stack([(R[0, k] * n[:, 0] + R[1, k] * n[:, 1]) + R[2, k] * n[:, 2] for k in range(3)], 1)   # R^T n
    Jr = np.stack([P64[:, 1] * u[:, 2] - P64[:, 2] * u[:, 1], P64[:, 2] * u[:, 0] - P64[:, 0] * u[:, 2],
                   P64[:, 0] * u[:, 1] - P64[:, 1] * u[:, 0]], 1)
    return r, np.concatenate([Jr, n], 1), W


def sums_of(r, J, inl, loss=None):
    """(H [6,6], g [6], cost, inliers) of the inliers' residuals, with first-order IRLS weights if a loss is set."""
    r, J = r[inl], J[inl]
    if loss is None or str(loss[0]).lower() == "trivial":
        rho, w = r * r, np.ones(len(r))
    else:
        rr = rho_vec(str(loss[0]).lower(), float(loss[1]), r * r)
        rho, w = rr[:, 0], rr[:, 1]
    H = (J * w[:, None]).T @ J
    g = (J * w[:, None]).T @ r
    return H, g, float(rho.sum()), int(inl.sum())


def linearize(surf, vs, T, P, max_distance, loss=None):
    W = world_points(T, P)
    plane, found = associate(surf, vs, W)
    r, J, _ = residuals(T, P, plane)
    inl = found & (np.abs(r) <= max_distance)
    H, g, cost, n = sums_of(r, J, inl, loss)
    q = W / (vs / 4.0)
    margin = float(np.min(np.abs(q - np.round(q))) * (vs / 4.0)) if len(W) else np.inf
    if found.any():
        margin = min(margin, float(np.min(np.abs(np.abs(r[found]) - max_distance))))
    return dict(H=H, g=g, cost=cost, inliers=n, margin=margin, r=r, J=J, inl=inl, plane=plane, found=found)


def register(surf, vs, T0, P, max_iterations=30, max_distance=0.1, min_inliers=100, min_eigenvalue=1e-3, tol_rot=1e-6,
             tol_pos=1e-6, loss=None):
    """Gauss-Newton as the device runs it.  Returns dict(pose, status, iterations, inliers, cost_first, cost_last, rmse,
    min_eigenvalue, information, trace) with trace[k] = dict(pose (at the linearisation), inliers, cost, margin, step)."""
    T = np.asarray(T0, np.float64).reshape(12).copy()
    out = dict(status=MAX_ITERATIONS, iterations=0, inliers=0, points=len(P), cost_first=0.0, cost_last=0.0, rmse=0.0,
               min_eigenvalue=0.0, information=np.zeros((6, 6)), trace=[])
    for it in range(max_iterations):
        lin = linearize(surf, vs, T, P, max_distance, loss)
        out["iterations"] = it + 1
        out["inliers"], out["cost_last"], out["information"] = lin["inliers"], lin["cost"], lin["H"]
        if it == 0:
            out["cost_first"] = lin["cost"]
        rec = dict(pose=T.copy(), inliers=lin["inliers"], cost=lin["cost"], margin=lin["margin"], step=None)
        out["trace"].append(rec)
        if lin["inliers"] < max(min_inliers, 1):
            out["status"] = TOO_FEW_INLIERS
            break
        out["rmse"] = float(np.sqrt(lin["cost"] / lin["inliers"]))
        out["min_eigenvalue"] = float(np.linalg.eigvalsh(lin["H"] / lin["inliers"])[0])
        if out["min_eigenvalue"] < min_eigenvalue:
            out["status"] = DEGENERATE
            break
        dx = -np.linalg.solve(lin["H"], lin["g"])
        rec["step"] = dx
        if np.linalg.norm(dx[:3]) <= tol_rot and np.linalg.norm(dx[3:]) <= tol_pos:
            out["status"] = CONVERGED
            break
        T = retract(T, dx)
    out["pose"] = T
    return out


def pose_error(T, Tgt):
    """(angle [rad], distance [m]) between two poses."""
    T, Tgt = np.asarray(T).reshape(12), np.asarray(Tgt).reshape(12)
    dR = T[:9].reshape(3, 3).T @ Tgt[:9].reshape(3, 3)
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(T[9:] - Tgt[9:]))


def perturb(T, rot, trans, seed):
    """T with a rotation of `rot` rad about a random axis (on the right) and a translation of `trans` m in a random direction."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3)
    dt /= np.linalg.norm(dt)
    return retract(T, np.r_[rot * ax, trans * dt])
