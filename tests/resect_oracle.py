"""numpy restatement of the camera resectioning (include/lvba_hip.h, "camera resectioning from 2-D to 3-D matches"; DESIGN.md
§10n): verify_oracle's generator and sampler keyed on (seed, id, -1, h), the three-point solver in csrc/resect_device.h's order of
operations (numpy rounds every product and every sum on its own, as a build without contraction does), the inlier test, the
choice.  All hypotheses of a job are one array.  The refinement is independent: the same residual over the same inliers minimised
to convergence with numpy.linalg (Rodrigues' formula, least squares), compared under a measured tolerance.  This is the project's
own definition; it is not pinned against COLMAP."""
import numpy as np

import match_oracle as mo
import verify_oracle as vo

OK, TOO_FEW_MATCHES, NO_MODEL, TOO_FEW_INLIERS = 0, 1, 2, 3
K = 4
MIN_DEPTH = 1e-12
TRIANGLE_REL2 = 1e-12
SPLIT_REL = 1e-14
NEWTON, POLISH = 16, 3
DEFAULTS = dict(hypotheses=1024, refine_rounds=2, min_inliers=30, max_error_px=8.0, seed=0)


def pack(xy, world):
    """records [m, 5] = (x, y, X): an unusable correspondence becomes (NaN, NaN, 0, 0, 0)"""
    xy, world = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(world, np.float64).reshape(-1, 3)
    ok = ~np.isnan(xy).any(axis=1) & np.isfinite(world).all(axis=1)
    rec = np.zeros((len(xy), 5))
    rec[:, :2] = np.where(ok[:, None], xy, np.nan)
    rec[:, 2:] = np.where(ok[:, None], world, 0.0)
    return rec


def records(intr, uv, world):
    return pack(mo.undistort_all(intr, uv), world)


def sample(seed, job_id, H, m):
    return vo.sample(seed, job_id, 0xFFFFFFFF, H, m, K)


def transform(R, t, X):
    """Xc of every (pose, point): R [H, 9], t [H, 3], X [m, 3] -> three [H, m] arrays"""
    R, t = np.asarray(R, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 3)
    X0, X1, X2 = (X[None, :, k] for k in range(3))
    r = [R[:, k][:, None] for k in range(9)]
    cx = ((r[0] * X0 + r[1] * X1) + r[2] * X2) + t[:, 0][:, None]
    cy = ((r[3] * X0 + r[4] * X1) + r[5] * X2) + t[:, 1][:, None]
    cz = ((r[6] * X0 + r[7] * X1) + r[8] * X2) + t[:, 2][:, None]
    return cx, cy, cz


def score(R, t, rec, intr, rho, with_margin=False):
    """bool [H, m] (or [m] for one pose): the inlier test"""
    one = np.ndim(R) == 1 or np.shape(R) == (3, 3)
    fx, fy = float(intr[0]), float(intr[1])
    with np.errstate(all="ignore"):
        cx, cy, cz = transform(R, t, rec[:, 2:5])
        x, y = rec[None, :, 0], rec[None, :, 1]
        a = fx * (cx - x * cz)
        b = fy * (cy - y * cz)
        r = float(rho) * cz
        lhs, rhs = a * a + b * b, r * r
        ok = (cz > MIN_DEPTH) & (lhs <= rhs)
    if not with_margin:
        return ok[0] if one else ok
    with np.errstate(all="ignore"):
        fin = np.isfinite(lhs) & np.isfinite(rhs) & (rhs > 0)
        rel = np.where(fin, np.abs(lhs - rhs) / np.where(fin, rhs, 1.0), np.inf)
        rel = np.minimum(rel, np.where(np.isfinite(cz), np.abs(cz - MIN_DEPTH) / MIN_DEPTH, np.inf))
    return (ok[0], rel[0]) if one else (ok, rel)


def _cof(A):
    return [A[3] * A[5] - A[4] * A[4], A[4] * A[2] - A[1] * A[5], A[1] * A[4] - A[3] * A[2], A[0] * A[5] - A[2] * A[2],
            A[1] * A[2] - A[0] * A[4], A[0] * A[3] - A[1] * A[1]]


def _det(A, C):
    return (A[0] * C[0] + A[1] * C[1]) + A[2] * C[2]


def _dot(C, B):
    return ((C[0] * B[0] + C[3] * B[3]) + C[5] * B[5]) + 2.0 * ((C[1] * B[1] + C[2] * B[2]) + C[4] * B[4])


def _form(A, u, v):
    w0 = (A[0] * v[0] + A[1] * v[1]) + A[2] * v[2]
    w1 = (A[1] * v[0] + A[3] * v[1]) + A[4] * v[2]
    w2 = (A[2] * v[0] + A[4] * v[1]) + A[5] * v[2]
    return (u[0] * w0 + u[1] * w1) + u[2] * w2


def _inv3(m):
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    return [c00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
            c01 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
            c02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det]


def _side(si, sj, b):
    return (si * si + sj * sj) - (2.0 * b) * (si * sj)


def _margin(value, ref):
    """|value| / ref where both are finite and ref > 0, else inf: how far a threshold `value > 0` is from flipping"""
    with np.errstate(all="ignore"):
        fin = np.isfinite(value) & np.isfinite(ref) & (ref > 0)
        return np.where(fin, np.abs(value) / np.where(fin, ref, 1.0), np.inf)


def p3p(S, fx, fy):
    """S [H, 4, 5] -> (R [H, 9], t [H, 3], valid [H], margin [H]): resect_p3p for every hypothesis at once.  margin: the smallest
    relative distance of a threshold the hypothesis met from its bound (over the ones it reached while still valid).  Covered:
    the triangle test, the cubic's leading coefficient, the sign of disc and the side Newton starts from, the split, each plane's
    discriminant, the depths' signs, the fourth point's depth.  NOT covered: the selections among computed values -- the largest
    B_ii, |N_rc| and |n_k|, and the smallest fourth-point error, each with its lowest-index rule --, which compare two results
    of the same arithmetic and need no distance from a constant while that arithmetic is the same bits everywhere."""
    H = len(S)
    fx, fy = float(fx), float(fy)
    with np.errstate(all="ignore"):
        c = [[S[:, j, k] for k in range(5)] for j in range(4)]
        valid = ~np.isnan(S[:, :, 0]).any(axis=1)
        margin = np.full(H, np.inf)

        def gate(cond, value, ref):
            nonlocal valid, margin
            margin = np.where(valid, np.minimum(margin, _margin(value, ref)), margin)
            valid = valid & cond

        f = []
        for j in range(3):
            n = np.sqrt((c[j][0] * c[j][0] + c[j][1] * c[j][1]) + 1.0)
            f += [c[j][0] / n, c[j][1] / n, 1.0 / n]
        b12 = (f[0] * f[3] + f[1] * f[4]) + f[2] * f[5]
        b13 = (f[0] * f[6] + f[1] * f[7]) + f[2] * f[8]
        b23 = (f[3] * f[6] + f[4] * f[7]) + f[5] * f[8]
        d12 = [c[0][2 + k] - c[1][2 + k] for k in range(3)]
        d13 = [c[0][2 + k] - c[2][2 + k] for k in range(3)]
        d23 = [c[1][2 + k] - c[2][2 + k] for k in range(3)]
        a12 = (d12[0] * d12[0] + d12[1] * d12[1]) + d12[2] * d12[2]
        a13 = (d13[0] * d13[0] + d13[1] * d13[1]) + d13[2] * d13[2]
        a23 = (d23[0] * d23[0] + d23[1] * d23[1]) + d23[2] * d23[2]
        cr = [d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0]]
        cc = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]
        tri = TRIANGLE_REL2 * (a12 * a13)
        gate(cc > tri, cc - tri, tri)
        zero = np.zeros(H)
        D1 = [a23, -(a23 * b12), zero, a23 - a12, a12 * b23, -a12]
        D2 = [a23, zero, -(a23 * b13), -a13, a13 * b23, a23 - a13]
        C1, C2 = _cof(D1), _cof(D2)
        k0, k1, k2, k3 = _det(D1, C1), _dot(C1, D2), _dot(C2, D1), _det(D2, C2)
        kscale = (np.abs(D2[0] * C2[0]) + np.abs(D2[1] * C2[1])) + np.abs(D2[2] * C2[2])      # the terms k3 is the sum of
        gate(k3 != 0.0, k3, kscale)
        b, cq, d = k2 / k3, k1 / k3, k0 / k3
        disc = b * b - 3.0 * cq
        gate(valid, disc, b * b + np.abs(3.0 * cq))          # the branch of the start (no condition of validity)
        v = np.sqrt(disc)
        t1 = (-b - v) / 3.0
        p1 = ((t1 + b) * t1 + cq) * t1 + d
        t2 = (v - b) / 3.0
        p2 = ((t2 + b) * t2 + cq) * t2 + d
        side = np.where(disc > 0.0, _margin(p1, (np.abs(t1 * t1 * t1) + np.abs(b * t1 * t1)) + (np.abs(cq * t1) + np.abs(d))), np.inf)
        margin = np.where(valid, np.minimum(margin, side), margin)        # the side Newton starts from
        g = np.where(disc > 0.0, np.where(p1 > 0.0, t1 - np.sqrt(p1 / v), t2 + np.sqrt(-p2 / v)), -b / 3.0)
        for _ in range(NEWTON):
            p = ((g + b) * g + cq) * g + d
            dp = (3.0 * g + 2.0 * b) * g + cq
            g = g - np.where(dp != 0.0, p / dp, 0.0)
        valid = valid & np.isfinite(g)
        D0 = [D1[k] + g * D2[k] for k in range(6)]
        C = _cof(D0)
        scale = np.abs(D0[0])
        for k in range(1, 6):
            scale = np.where(np.abs(D0[k]) > scale, np.abs(D0[k]), scale)
        B = [-C[0], -C[3], -C[5]]
        i = np.zeros(H, np.int64)
        bb = B[0]
        i = np.where(B[1] > bb, 1, i); bb = np.where(B[1] > bb, B[1], bb)
        i = np.where(B[2] > bb, 2, i); bb = np.where(B[2] > bb, B[2], bb)
        thr = SPLIT_REL * (scale * scale)
        gate(bb > thr, bb - thr, thr)
        sb = np.sqrt(bb)
        col = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
        pv = [-np.where(i == 0, col[0][j], np.where(i == 1, col[1][j], col[2][j])) / sb for j in range(3)]
        N = [D0[0], D0[1] - pv[2], D0[2] + pv[1], D0[1] + pv[2], D0[3], D0[4] - pv[0], D0[2] - pv[1], D0[4] + pv[0], D0[5]]
        best = np.full(H, -1.0)
        nA, nB = [zero] * 3, [zero] * 3
        for r in range(3):
            for cc_ in range(3):
                a = np.abs(N[3 * r + cc_])
                up = a > best
                best = np.where(up, a, best)
                nA = [np.where(up, N[3 * r + k], nA[k]) for k in range(3)]
                nB = [np.where(up, N[3 * k + cc_], nB[k]) for k in range(3)]
        valid = valid & (best > 0.0)
        Xi = _inv3([d12[0], d13[0], cr[0], d12[1], d13[1], cr[1], d12[2], d13[2], cr[2]])
        asum = (a12 + a13) + a23
        best_err = np.full(H, np.inf)
        found = np.zeros(H, bool)
        R, t = np.zeros((H, 9)), np.zeros((H, 3))
        X1 = [c[0][2], c[0][3], c[0][4]]
        for n in (nA, nB):
            k = np.zeros(H, np.int64)
            nb = np.abs(n[0])
            k = np.where(np.abs(n[1]) > nb, 1, k); nb = np.where(np.abs(n[1]) > nb, np.abs(n[1]), nb)
            k = np.where(np.abs(n[2]) > nb, 2, k)
            u = [np.where(k == 0, -n[1], np.where(k == 1, n[1], n[2])), np.where(k == 0, n[0], np.where(k == 1, -n[0], 0.0)),
                 np.where(k == 2, -n[0], 0.0)]
            w = [np.where(k == 0, -n[2], 0.0), np.where(k == 0, 0.0, np.where(k == 1, -n[2], n[2])),
                 np.where(k == 0, n[0], np.where(k == 1, n[1], -n[1]))]
            qa, qb, qc = _form(D1, u, u), _form(D1, u, w), _form(D1, w, w)
            qd = qb * qb - qa * qc
            plane_ok = valid & (qd >= 0.0)
            margin = np.where(valid, np.minimum(margin, _margin(qd, qb * qb + np.abs(qa * qc))), margin)
            sq = np.sqrt(qd)
            q = np.where(qb >= 0.0, (-qb) - sq, sq - qb)
            for root in range(2):
                al, be = (q, qa) if root == 0 else (qc, q)
                s0, s1, s2 = al * u[0] + be * w[0], al * u[1] + be * w[1], al * u[2] + be * w[2]
                ww = (_side(s0, s1, b12) + _side(s0, s2, b13)) + _side(s1, s2, b23)
                lam = np.sqrt(asum / ww)
                lam = np.where(s0 < 0.0, -lam, lam)
                s0, s1, s2 = lam * s0, lam * s1, lam * s2
                for _ in range(POLISH):
                    h0, h1, h2 = 0.5 * (_side(s0, s1, b12) - a12), 0.5 * (_side(s0, s2, b13) - a13), 0.5 * (_side(s1, s2, b23) - a23)
                    Ji = _inv3([s0 - b12 * s1, s1 - b12 * s0, zero, s0 - b13 * s2, zero, s2 - b13 * s0, zero, s1 - b23 * s2, s2 - b23 * s1])
                    s0, s1, s2 = (s0 - ((Ji[0] * h0 + Ji[1] * h1) + Ji[2] * h2), s1 - ((Ji[3] * h0 + Ji[4] * h1) + Ji[5] * h2),
                                  s2 - ((Ji[6] * h0 + Ji[7] * h1) + Ji[8] * h2))
                sol = plane_ok & (s0 > 0.0) & (s1 > 0.0) & (s2 > 0.0) & np.isfinite(s0) & np.isfinite(s1) & np.isfinite(s2)
                smax = np.maximum(np.maximum(np.abs(s0), np.abs(s1)), np.abs(s2))
                margin = np.where(plane_ok, np.minimum(margin, _margin(np.minimum(np.minimum(np.abs(s0), np.abs(s1)), np.abs(s2)), smax)), margin)
                y0, y1, y2 = [s0 * f[k] for k in range(3)], [s1 * f[3 + k] for k in range(3)], [s2 * f[6 + k] for k in range(3)]
                e1, e2 = [y0[k] - y1[k] for k in range(3)], [y0[k] - y2[k] for k in range(3)]
                e3 = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                Rs = [(e1[r] * Xi[cc_] + e2[r] * Xi[3 + cc_]) + e3[r] * Xi[6 + cc_] for r in range(3) for cc_ in range(3)]
                ts = [y0[r] - ((Rs[3 * r] * X1[0] + Rs[3 * r + 1] * X1[1]) + Rs[3 * r + 2] * X1[2]) for r in range(3)]
                X4 = [c[3][2], c[3][3], c[3][4]]
                px = ((Rs[0] * X4[0] + Rs[1] * X4[1]) + Rs[2] * X4[2]) + ts[0]
                py = ((Rs[3] * X4[0] + Rs[4] * X4[1]) + Rs[5] * X4[2]) + ts[1]
                pz = ((Rs[6] * X4[0] + Rs[7] * X4[1]) + Rs[8] * X4[2]) + ts[2]
                margin = np.where(sol, np.minimum(margin, _margin(pz - MIN_DEPTH, np.abs(pz) + MIN_DEPTH)), margin)
                sol = sol & (pz > MIN_DEPTH)
                ex, ey = fx * (px / pz - c[3][0]), fy * (py / pz - c[3][1])
                err = ex * ex + ey * ey
                up = sol & (err < best_err)
                best_err = np.where(up, err, best_err)
                found = found | up
                for e in range(9):
                    R[:, e] = np.where(up, Rs[e], R[:, e])
                for e in range(3):
                    t[:, e] = np.where(up, ts[e], t[:, e])
        valid = valid & found
        R[~valid] = 0.0
        t[~valid] = 0.0
    return R, t, valid, margin


def hypotheses(rec, job_id, intr, with_margin=False, **kw):
    """(R [H, 9], t [H, 3], count [H], idx [H, 4]) of every hypothesis of a job with records rec [m, 5]; invalid: zeros, -1"""
    o = dict(DEFAULTS, **kw)
    H, m = int(o["hypotheses"]), len(rec)
    if m < K:
        out = np.zeros((H, 9)), np.zeros((H, 3)), np.full(H, -1, np.int64), np.zeros((H, K), np.int64)
        return out + (np.inf,) if with_margin else out
    idx = sample(o["seed"], job_id, H, m)
    R, t, valid, pm = p3p(rec[idx], intr[0], intr[1])
    margin = float(pm.min(initial=np.inf))
    count = np.full(H, -1, np.int64)
    step = max(1, (1 << 21) // max(m, 1))
    for h0 in range(0, H, step):
        res = score(R[h0:h0 + step], t[h0:h0 + step], rec, intr, o["max_error_px"], with_margin)
        ok = res[0] if with_margin else res
        if with_margin and valid[h0:h0 + step].any():
            margin = min(margin, float(res[1][valid[h0:h0 + step]].min(initial=np.inf)))
        count[h0:h0 + step] = ok.sum(axis=1)
    count[~valid] = -1
    return (R, t, count, idx, margin) if with_margin else (R, t, count, idx)


pick = vo.pick


def rodrigues(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def nearest_rotation(R):
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def residuals(R, t, rec, intr):
    """[n, 2] in undistorted pixels"""
    Xc = rec[:, 2:5] @ np.asarray(R).reshape(3, 3).T + np.asarray(t).reshape(3)
    return np.stack([intr[0] * (Xc[:, 0] / Xc[:, 2] - rec[:, 0]), intr[1] * (Xc[:, 1] / Xc[:, 2] - rec[:, 1])], 1)


def jacobian(R, t, rec, intr):
    """[n, 2, 6] by (om, up) of Xc <- Xc + om x Xc + up, analytic (information() is checked against finite differences)"""
    Xc = rec[:, 2:5] @ np.asarray(R).reshape(3, 3).T + np.asarray(t).reshape(3)
    X, Y, Z = Xc.T
    J = np.zeros((len(rec), 2, 6))
    gx, gy = intr[0] / Z, intr[1] / Z
    dr = np.zeros((len(rec), 2, 3))
    dr[:, 0, 0], dr[:, 0, 2] = gx, -gx * X / Z
    dr[:, 1, 1], dr[:, 1, 2] = gy, -gy * Y / Z
    sk = np.zeros((len(rec), 3, 3))                       # -[Xc]x
    sk[:, 0, 1], sk[:, 0, 2], sk[:, 1, 0], sk[:, 1, 2], sk[:, 2, 0], sk[:, 2, 1] = Z, -Y, -Z, X, Y, -X
    J[:, :, :3] = dr @ sk
    J[:, :, 3:] = dr
    return J


def fit(R, t, rec, intr, iters=30):
    """the pose that minimises the squared residuals over rec, from (R, t): Gauss-Newton with lstsq to convergence; None where
    the system is rank deficient"""
    R, t = nearest_rotation(R), np.asarray(t, np.float64).reshape(3).copy()
    if len(rec) < 3:
        return None
    for _ in range(iters):
        r = residuals(R, t, rec, intr).reshape(-1)
        J = jacobian(R, t, rec, intr).reshape(-1, 6)
        if not (np.isfinite(r).all() and np.isfinite(J).all()) or np.linalg.matrix_rank(J) < 6:
            return None
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        dR = rodrigues(d[:3])
        R, t = dR @ R, dR @ t + d[3:]
        if np.abs(d).max() < 1e-15:
            break
    return R.reshape(9), t


def information(R, t, rec, intr):
    J = jacobian(R, t, rec, intr).reshape(-1, 6)
    return J.T @ J


def information_fd(R, t, rec, intr, step):
    """sum J^T J with J by central finite differences of residuals() in the left perturbation"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    J = np.zeros((2 * len(rec), 6))
    for k in range(6):
        d = np.zeros(6); d[k] = step
        out = []
        for s in (1.0, -1.0):
            dR = rodrigues(s * d[:3])
            out.append(residuals(dR @ R, dR @ t + s * d[3:], rec, intr).reshape(-1))
        J[:, k] = (out[0] - out[1]) / (2 * step)
    return J.T @ J


def resect(rec, job_id, intr, **kw):
    """dict(R [9], t [3], status, n_inliers, best_h, mask [m], rmse_px, information [6, 6], R0, t0, count0) of one job; mask is
    all False unless the status is OK; R0, t0, count0 the winning hypothesis"""
    o = dict(DEFAULTS, **kw)
    m = len(rec)
    out = dict(R=np.zeros(9), t=np.zeros(3), status=TOO_FEW_MATCHES, n_inliers=0, best_h=-1, mask=np.zeros(m, bool), rmse_px=0.0,
               information=np.zeros((6, 6)), R0=np.zeros(9), t0=np.zeros(3), count0=0)
    if m < max(K, o["min_inliers"]):
        return out
    R, t, count, _ = hypotheses(rec, job_id, intr, **o)
    h, c = pick(count)
    if h < 0:
        out["status"] = NO_MODEL
        return out
    rho = o["max_error_px"]
    bR, bt = R[h], t[h]
    out.update(R0=bR.copy(), t0=bt.copy(), count0=c)
    for _ in range(int(o["refine_rounds"])):
        if c <= 0:
            break
        res = fit(bR, bt, rec[score(bR, bt, rec, intr, rho)], intr)
        if res is None:
            break
        cn = int(score(res[0], res[1], rec, intr, rho).sum())
        if cn < c:
            break
        bR, bt, c = res[0], res[1], cn
    inl = score(bR, bt, rec, intr, rho)
    out.update(R=bR, t=bt, n_inliers=c, best_h=h, status=OK if c >= o["min_inliers"] else TOO_FEW_INLIERS)
    if c > 0:
        r = residuals(bR, bt, rec[inl], intr)
        out.update(rmse_px=float(np.sqrt((r * r).sum() / c)), information=information(bR, bt, rec[inl], intr))
    if out["status"] == OK:
        out["mask"] = inl
    return out


def pose_difference(R, t, R2, t2):
    """(Frobenius norm of R - R2, |t - t2| / |t2|)"""
    dR = float(np.linalg.norm(np.asarray(R).reshape(9) - np.asarray(R2).reshape(9)))
    n = float(np.linalg.norm(t2))
    return dR, float(np.linalg.norm(np.asarray(t).reshape(3) - np.asarray(t2).reshape(3))) / (n if n > 0 else 1.0)


def pose_offset(R, t, R2, t2):
    """(rotation angle in degrees, distance of the camera centres) between two poses T_cam<-world"""
    R, R2 = np.asarray(R, np.float64).reshape(3, 3), np.asarray(R2, np.float64).reshape(3, 3)
    c = 0.5 * (np.trace(R @ R2.T) - 1.0)
    ang = float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    return ang, float(np.linalg.norm(-R.T @ np.asarray(t).reshape(3) + R2.T @ np.asarray(t2).reshape(3)))
