"""numpy restatement of the homography model of the two-view verification and of the E-or-H choice (include/lvba_hip.h, "The
homography model and the E-or-H choice"): the 8 x 9 system of four matches, its null vector in
csrc/verify_device.h's order of operations (verify_eight_solve as it stands), the sign, the adjugate, the symmetric transfer gate
with its margins, the refit (LAPACK eigh, compared under a measured tolerance), a pair and the choice between the two models.
The sampler, `unit`, `points` and the essential side are verify_oracle's.  All hypotheses of a pair are one array.  This is the
project's own definition; it is not pinned against COLMAP."""
import numpy as np

import match_oracle as mo
import verify_oracle as vo

K = 4
ESSENTIAL, HOMOGRAPHY, AUTO = 0, 1, 2
MODEL_NAMES = ("essential", "homography", "auto")
PLANAR_RATIO = 0.8


def rows(P):
    """[..., 2, 9]: the two rows of each match (x_lo, y_lo, x_hi, y_hi) in the system"""
    xl, yl, xh, yh = (P[..., k] for k in range(4))
    one, zero = np.ones_like(xl), np.zeros_like(xl)
    r1 = np.stack([xl, yl, one, zero, zero, zero, -xh * xl, -xh * yl, -xh], -1)
    r2 = np.stack([zero, zero, zero, xl, yl, one, -yh * xl, -yh * yl, -yh], -1)
    return np.stack([r1, r2], -2)


def null_vector(A, bad):
    """A [H, 8, 9] -> (v [H, 9] of unit norm, valid [H]): verify_eight_solve for every hypothesis at once"""
    H = len(A)
    A = A.copy()
    A[bad] = 0.0
    scale = np.abs(A).reshape(H, 72).max(axis=1)
    perm = np.tile(np.arange(9), (H, 1))
    valid = ~bad
    ar = np.arange(H)
    with np.errstate(all="ignore"):
        for s in range(8):
            flat = np.abs(A[:, s:, s:]).reshape(H, -1)
            k = flat.argmax(axis=1)                   # the first of equals: the lowest (row, column)
            valid &= flat[ar, k] > vo.PIVOT_REL * scale
            pr, pc = s + k // (9 - s), s + k % (9 - s)
            row = A[ar, s].copy(); A[ar, s] = A[ar, pr]; A[ar, pr] = row
            col = A[ar, :, s].copy(); A[ar, :, s] = A[ar, :, pc]; A[ar, :, pc] = col
            name = perm[ar, s].copy(); perm[ar, s] = perm[ar, pc]; perm[ar, pc] = name
            A[:, s, s + 1:] = A[:, s, s + 1:] / A[:, s, s][:, None]
            for r in range(8):
                if r != s:
                    f = A[:, r, s].copy()
                    A[:, r, s + 1:] = A[:, r, s + 1:] - f[:, None] * A[:, s, s + 1:]
        v = np.concatenate([-A[:, :, 8], np.ones((H, 1))], 1)
        E = np.zeros((H, 9))
        E[ar[:, None], perm] = v
        E, ok = vo.unit(E)
    valid &= ok
    E[~valid] = 0.0
    return E, valid


def inverse(Hm, with_margin=False):
    """Hm [H, 9] -> (G [H, 9] = adj(H), negated where det H < 0, ok [H]); G = 0 where det H is 0 or not finite"""
    h = [Hm[:, k] for k in range(9)]
    with np.errstate(all="ignore"):
        G = np.stack([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                      h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                      h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]], 1)
        t = [h[0] * G[:, 0], h[1] * G[:, 3], h[2] * G[:, 6]]
        det = (t[0] + t[1]) + t[2]
        ok = np.isfinite(det) & (det != 0.0)
        G = np.where((det < 0.0)[:, None], -G, G)
        G[~ok] = 0.0
        if not with_margin:
            return G, ok
        size = (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])
        rel = np.where(ok & (size > 0), np.abs(det) / np.where(size > 0, size, 1.0), np.inf)
    return G, ok, rel


def homography(S, with_margin=False):
    """S [H, 4, 4] -> (Hm [H, 9], G [H, 9], valid [H]): rows, solve, sign, inverse direction; invalid: Hm = G = 0"""
    H = len(S)
    bad = np.isnan(S).any(axis=(1, 2))
    A = rows(S).reshape(H, 8, 9)
    Hm, valid = null_vector(A, bad)
    with np.errstate(all="ignore"):
        xl, yl = S[:, 0, 0], S[:, 0, 1]
        t = [Hm[:, 6] * xl, Hm[:, 7] * yl, Hm[:, 8]]
        p2 = (t[0] + t[1]) + t[2]
        size = (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])
        sign_rel = np.where(valid & (size > 0), np.abs(p2) / np.where(size > 0, size, 1.0), np.inf)
    valid &= (p2 > 0.0) | (p2 < 0.0)
    Hm = np.where((p2 < 0.0)[:, None], -Hm, Hm)
    Hm[~valid] = 0.0
    G, ok, det_rel = inverse(Hm, with_margin=True)
    det_rel = np.where(valid, det_rel, np.inf)
    valid &= ok
    Hm[~valid] = 0.0
    G[~valid] = 0.0
    if with_margin:
        m = min(sign_rel[valid].min(initial=np.inf), det_rel[valid].min(initial=np.inf))
        return Hm, G, valid, m
    return Hm, G, valid


def transfer(M, x, y, u, v, tau2):
    """(ok, relative margin) [H, m] of one direction: (x, y, 1) carried by M [H, 9] lands within tau of (u, v), in front"""
    e = [M[:, k][:, None] for k in range(9)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = [e[6] * x, e[7] * y, e[8]]
        p0 = (e[0] * x + e[1] * y) + e[2]
        p1 = (e[3] * x + e[4] * y) + e[5]
        p2 = (t[0] + t[1]) + t[2]
        d0, d1 = p0 - u * p2, p1 - v * p2
        e2 = d0 * d0 + d1 * d1
        bound = tau2 * (p2 * p2)
        ok = (e2 <= bound) & (p2 > 0.0)
        fin = np.isfinite(e2) & np.isfinite(bound) & (bound > 0)
        rel = np.where(fin, np.abs(e2 - bound) / np.where(fin, bound, 1.0), np.inf)
        size = (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])
        fin = np.isfinite(p2) & (size > 0)
        rel = np.minimum(rel, np.where(fin, np.abs(p2) / np.where(fin, size, 1.0), np.inf))
    return ok, rel


def score(Hm, P, tau2, with_margin=False, G=None):
    """bool [H, m] (or [m] for one H): the symmetric transfer test; all False where H has no inverse direction"""
    one = np.ndim(Hm) == 1 or np.shape(Hm) == (3, 3)
    Hm = np.asarray(Hm, np.float64).reshape(-1, 9)
    if G is None:
        G, _ = inverse(Hm)
    xl, yl, xh, yh = (P[None, :, k] for k in range(4))
    ok1, r1 = transfer(Hm, xl, yl, xh, yh, tau2)
    ok2, r2 = transfer(G, xh, yh, xl, yl, tau2)
    ok, rel = ok1 & ok2, np.minimum(r1, r2)
    if one:
        ok, rel = ok[0], rel[0]
    return (ok, rel) if with_margin else ok


def hypotheses(P, lo, hi, with_margin=False, **kw):
    """(Hm [H, 9], count [H], idx [H, 4]) of every hypothesis of a pair with points P [m, 4]; invalid: Hm = 0, count = -1"""
    o = dict(vo.DEFAULTS, **kw)
    H, m = int(o["hypotheses"]), len(P)
    if m < K:
        out = np.zeros((H, 9)), np.full(H, -1, np.int64), np.zeros((H, K), np.int64)
        return out + (np.inf,) if with_margin else out
    idx = vo.sample(o["seed"], lo, hi, H, m, K)
    Hm, G, valid, margin = homography(P[idx], with_margin=True)
    tau2 = mo.tau2(o["intr"], o["max_error_px"])
    count = np.full(H, -1, np.int64)
    step = max(1, (1 << 21) // max(m, 1))
    for h0 in range(0, H, step):
        ok, rel = score(Hm[h0:h0 + step], P, tau2, True, G=G[h0:h0 + step])
        v = valid[h0:h0 + step]
        if v.any():
            margin = min(margin, rel[v].min(initial=np.inf))
        count[h0:h0 + step] = ok.sum(axis=1)
    count[~valid] = -1
    return (Hm, count, idx, margin) if with_margin else (Hm, count, idx)


def refit(Hm, P, tau2):
    """the refit of H over its inliers with LAPACK; None where there is none"""
    Hm = np.asarray(Hm, np.float64).reshape(9)
    Q = P[score(Hm, P, tau2)]
    if not len(Q):
        return None
    A = rows(Q).reshape(-1, 9)
    w, v = np.linalg.eigh(A.T @ A)
    F = v[:, 0]
    n = np.linalg.norm(F)
    if not (n > 0 and np.isfinite(n)):
        return None
    F = F / n
    if F @ Hm < 0:
        F = -F
    return F if inverse(F[None, :])[1][0] else None


def verify_pair(P, lo, hi, **kw):
    """dict(E [9] (the homography), status, n_inliers, best_h, mask [m]) of one pair; mask is all False unless the status is OK"""
    o = dict(vo.DEFAULTS, **kw)
    m = len(P)
    out = dict(E=np.zeros(9), status=vo.TOO_FEW_MATCHES, n_inliers=0, best_h=-1, mask=np.zeros(m, bool))
    if m < max(K, o["min_inliers"]):
        return out
    Hm, count, _ = hypotheses(P, lo, hi, **o)
    h, c = vo.pick(count)
    if h < 0:
        out["status"] = vo.NO_MODEL
        return out
    tau2 = mo.tau2(o["intr"], o["max_error_px"])
    best = Hm[h]
    for _ in range(int(o["refine_rounds"])):
        if c <= 0:
            break
        F = refit(best, P, tau2)
        if F is None:
            break
        cn = int(score(F, P, tau2).sum())
        if cn <= c:
            break
        best, c = F, cn
    out.update(E=best, n_inliers=c, best_h=h, status=vo.OK if c >= o["min_inliers"] else vo.TOO_FEW_INLIERS)
    if out["status"] == vo.OK:
        out["mask"] = score(best, P, tau2)
    return out


def choose(rE, rH, planar_ratio=PLANAR_RATIO):
    """HOMOGRAPHY iff the H run is OK and either the E run is not OK or n_H >= planar_ratio n_E in fp64"""
    planar = rH["status"] == vo.OK and (rE["status"] != vo.OK or float(rH["n_inliers"]) >= float(planar_ratio) * float(rE["n_inliers"]))
    return HOMOGRAPHY if planar else ESSENTIAL


def verify_auto(rE, rH, planar_ratio=PLANAR_RATIO):
    """the chosen run's outputs with kind, n_inliers_E and n_inliers_H"""
    kind = choose(rE, rH, planar_ratio)
    return dict(rH if kind == HOMOGRAPHY else rE, kind=kind, n_inliers_E=rE["n_inliers"], n_inliers_H=rH["n_inliers"])
