"""Reference model of the LiDAR stage's robust losses (lvba_balm_set_loss).  TEST INFRASTRUCTURE, not product code.

Built on oracle/balm_oracle.py without changing it:
    C(x) = sum_v rho(lambda_min(v)) [+ priors],   g = sum_v rho'(s_v) g_v,   H = sum_v rho'(s_v) H_v
with (H_v, g_v, lambda_v) of ONE voxel from balm_oracle.acc_evaluate2 and rho from this file's own numpy restatement of the six kinds
(Ceres 2.1 loss_function.cc; tests/test_robust_balm_host.py holds it against csrc/visual_loss.h compiled for the host).  The
rho'' g_v g_v^T term is left out of H, as the library documents.  The robust LM is balm_oracle.damping_iter with its eval_fn /
cost_fn hooks set to these, so the control flow is the pinned one.
"""
import math

import numpy as np

from oracle import balm_oracle as bo

KINDS = {"trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}
DBL_MIN = 2.2250738585072014e-308


def rho(kind, a, s):
    """(rho, rho', rho'') at s for the loss `kind` of scale a (b = a^2)."""
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    a, s = float(a), float(s)
    b = a * a
    if k == 1:
        if s > b:
            r = math.sqrt(s)
            r1 = max(DBL_MIN, a / r)
            return 2.0 * a * r - b, r1, -r1 / (2.0 * s)
        return s, 1.0, 0.0
    if k == 2:
        c = 1.0 / b
        sm = 1.0 + s * c
        t = math.sqrt(sm)
        r1 = max(DBL_MIN, 1.0 / t)
        return 2.0 * b * (t - 1.0), r1, -(c * r1) / (2.0 * sm)
    if k == 3:
        c = 1.0 / b
        sm = 1.0 + s * c
        inv = 1.0 / sm
        return b * math.log(sm), max(DBL_MIN, inv), -c * (inv * inv)
    if k == 4:
        c = 1.0 / b
        sm = 1.0 + s * s * c
        inv = 1.0 / sm
        return a * math.atan2(s, a), max(DBL_MIN, inv), -2.0 * s * c * (inv * inv)
    if k == 5:
        if s <= b:
            v = 1.0 - s / b
            return b / 3.0 * (1.0 - v * v * v), v * v, -2.0 / b * v
        return b / 3.0, 0.0, 0.0
    return s, 1.0, 0.0


def problem(d):
    return bo.Problem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"])


def voxel_terms(prob, poses, v):
    """(H_v [6k, 6k], g_v [6k], lambda_v, poses of the voxel [k]) of voxel v: acc_evaluate2 on the voxel alone.  The voxel is handed
    over with its k observing poses renumbered 0..k-1 (ascending, as in the problem), which leaves every block acc_evaluate2
    forms unchanged and spares the 6N x 6N zeros around them."""
    f0, f1 = int(prob.voxel_off[v]), int(prob.voxel_off[v + 1])
    idx = np.asarray(prob.pose_idx[f0:f1])
    ps, loc = np.unique(idx, return_inverse=True)
    one = bo.Problem(len(ps), np.array([0, f1 - f0]), loc.astype(np.int32), prob.clusters[f0:f1])
    x = np.asarray(poses, np.float64).reshape(-1, 12)[ps]
    H, g, lam = bo.acc_evaluate2(one, x, 0, 1)
    return H, g, lam, ps


def evaluate(prob, poses, kind, a):
    """(H, g, cost SUM) of the robust voxel cost; also returns the per-voxel (lambda, weight)."""
    n = 6 * prob.n_poses
    H, g, c = np.zeros((n, n)), np.zeros(n), 0.0
    lam, w = np.zeros(prob.n_voxels), np.zeros(prob.n_voxels)
    for v in range(prob.n_voxels):
        Hv, gv, lv, ps = voxel_terms(prob, poses, v)
        r0, r1, _ = rho(kind, a, lv)
        ii = (6 * ps[:, None] + np.arange(6)[None, :]).reshape(-1)
        H[np.ix_(ii, ii)] += r1 * Hv
        g[ii] += r1 * gv
        c += r0
        lam[v], w[v] = lv, r1
    return H, g, c, lam, w


def cost(prob, poses, kind, a):
    """sum_v rho(lambda_min) from the vectorised eigenvalues (balm_oracle.voxel_lambdas)"""
    return float(sum(rho(kind, a, s)[0] for s in bo.voxel_lambdas(prob, poses)[:, 0]))


def lambdas_weights(prob, poses, kind, a):
    lam = bo.voxel_lambdas(prob, poses)[:, 0]
    return lam, np.array([rho(kind, a, s)[1] for s in lam])


def voxel_moment_scale(prob, poses):
    """M_v = max over the voxel's factors of (|p_f| + |v_f| / n_f)^2: the size, per point, of the second-moment terms that cancel
    down to lambda_min.  The pose transform forms R P R^T + (R v) p^T + p (R v)^T + n p p^T, whose terms are of size n |p|^2 and
    n |v / n|^2 whatever is left of them afterwards (a voxel near the world origin seen from a pose 100 m away: R v ~ -n p), and
    the merged centroid is no larger than that by the triangle inequality."""
    _, ps = bo.unpack_poses(poses)
    m = (np.linalg.norm(ps[prob.pose_idx], axis=1) + np.linalg.norm(prob.v, axis=1) / prob.n) ** 2
    return np.maximum.reduceat(m, prob.voxel_off[:-1])


def damping_iter(prob, poses, kind="trivial", a=1.0, priors=None, max_iter=10, u0=0.01, v0=2.0, rel_tol=1e-6):
    """balm_oracle.damping_iter on the robust quantities (+ the prior terms of tests/prior_oracle.py, outside the loss).  Solve:
    the C oracle's unpivoted dense LDL^T, the factorisation the GPU solvers perform."""
    import oracle
    V = prob.n_voxels
    priors = list(priors or [])
    if priors:
        import prior_oracle as po

    def ev(x):
        H, g, c, _, _ = evaluate(prob, x, kind, a)
        if priors:
            Hp, gp, cp = po.assemble(priors, x)
            H, g, c = H + Hp, g + gp, c + cp
        return H, g, c / V

    def cf(x):
        c = cost(prob, x, kind, a)
        if priors:
            c += po.assemble(priors, x)[2]
        return c / V

    def solve(A, b):
        x, rc = oracle.ldlt_solve_dense(A, b)
        assert rc == 0
        return x

    return bo.damping_iter(prob, poses, max_iter, u0, v0, rel_tol, eval_fn=ev, cost_fn=cf, solve_fn=solve)


def add_outlier_voxels(d, frac, seed, lo, hi):
    """A copy of the problem dict d in which, for a share `frac` of the voxels, ONE factor's cluster is moved by a body-frame
    vector delta with |delta| in [lo, hi]: v' = v + n delta, P' = P + v delta^T + delta v^T + n delta delta^T (exact on the
    second-moment statistics; no points needed).  Returns (problem dict, touched [V] bool)."""
    rng = np.random.default_rng(seed)
    off = np.asarray(d["voxel_off"])
    V = len(off) - 1
    clu = np.array(d["clusters"], np.float64).reshape(-1, 10).copy()
    touched = np.zeros(V, bool)
    touched[rng.choice(V, int(round(frac * V)), replace=False)] = True
    P, v, n = bo.unpack_clusters(clu)
    for a in np.nonzero(touched)[0]:
        f = int(rng.integers(off[a], off[a + 1]))
        u = rng.standard_normal(3)
        dl = u / np.linalg.norm(u) * rng.uniform(lo, hi)
        P[f] = P[f] + np.outer(v[f], dl) + np.outer(dl, v[f]) + n[f] * np.outer(dl, dl)
        v[f] = v[f] + n[f] * dl
    out = dict(d)
    out["clusters"] = bo.pack_clusters(P, v, n)
    return out, touched


def derive_scale(d, poses):
    """a with a^2 = 4 x the 90th percentile of lambda_min over the voxels of the (uncontaminated) problem d at `poses`"""
    lam = bo.voxel_lambdas(problem(d), poses)[:, 0]
    return math.sqrt(4.0 * float(np.percentile(lam, 90)))


def contaminated(d, seed=10, frac=0.25):
    """The standard input of the robust tests: (contaminated dict, touched, a).  The scale comes from the untouched voxels at
    the initial poses, the displacements lie between 5 a and 20 a.  A displacement lifts lambda_min only by its part along the
    voxel's normal, and never beyond the voxel's middle eigenvalue (a rank-one update interlaces), so about two in five displaced
    voxels end above a^2: the default seed is one for which the problems the tests use meet check_input_shares."""
    a = derive_scale(d, d["poses_init"])
    dc, touched = add_outlier_voxels(d, frac, seed, 5.0 * a, 20.0 * a)
    return dc, touched, a


def check_input_shares(dc, a):
    """The two conditions on the inputs every test asserts before it looks at the GPU: >= 10 % of the voxels above a^2,
    >= 75 % at or below it (oracle values at the initial poses)."""
    lam = bo.voxel_lambdas(problem(dc), dc["poses_init"])[:, 0]
    hi, lo = float(np.mean(lam > a * a)), float(np.mean(lam <= a * a))
    assert hi >= 0.10 and lo >= 0.75, (hi, lo)
    return hi, lo


def relative_to_first(poses):
    """every pose expressed relative to pose 0 (fixes the gauge): [N, 12]"""
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    R0, p0 = x[0, :9].reshape(3, 3), x[0, 9:]
    out = np.empty_like(x)
    for i, row in enumerate(x):
        out[i, :9] = (R0.T @ row[:9].reshape(3, 3)).reshape(9)
        out[i, 9:] = R0.T @ (row[9:] - p0)
    return out


def gauge_distance(xa, xb):
    """largest translation difference over the poses, both sets relative to their pose 0"""
    return float(np.linalg.norm(relative_to_first(xa)[:, 9:] - relative_to_first(xb)[:, 9:], axis=1).max())
