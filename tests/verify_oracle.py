"""numpy restatement of the two-view verification (include/lvba_hip.h, "two-view verification of putative matches"; DESIGN.md
§10k): the generator in uint64, the sampler, the two solvers in csrc/verify_device.h's order of operations (numpy rounds every
product and every sum on its own, as a build without contraction does), the gate in match_oracle's expressions, the choice.  All
hypotheses of a pair are one array.  The refits are restated with LAPACK (eigh, svd), not operation for operation: they are
compared under a measured tolerance.  This is the project's own definition; it is not pinned against COLMAP."""
import numpy as np

import match_oracle as mo

EIGHT_POINT, KNOWN_ROTATION = 0, 1
OK, TOO_FEW_MATCHES, NO_MODEL, TOO_FEW_INLIERS = 0, 1, 2, 3
PIVOT_REL = 1e-10
T_REL2 = 1e-20
DEFAULTS = dict(method=EIGHT_POINT, hypotheses=1024, refine_rounds=2, min_inliers=15, max_error_px=4.0, seed=0)
G = np.uint64(0x9E3779B97F4A7C15)
U = np.uint64


def sample_size(method):
    return 2 if method == KNOWN_ROTATION else 8


def mix(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def keys(seed, lo, hi, h):
    """h: an array of hypothesis numbers"""
    with np.errstate(over="ignore"):
        k = mix(U(seed) + G)
        k = mix(k ^ ((U(lo) << U(32)) | U(hi)))
        return mix(k + G * (np.asarray(h, np.uint64) + U(1)))


def draw(key, j):
    with np.errstate(over="ignore"):
        return mix(key + G * U(j + 1))


def below(r, n):
    """the high half of r n for n < 2^32, without 128-bit integers"""
    n = U(n)
    rh, rl = r >> U(32), r & U(0xFFFFFFFF)
    return ((rh * n + ((rl * n) >> U(32))) >> U(32)).astype(np.int64)


def sample(seed, lo, hi, H, m, k):
    """int64 [H, k]: the positions hypothesis h draws, in draw order"""
    key = keys(seed, lo, hi, np.arange(H))
    idx = np.zeros((H, k), np.int64)
    for j in range(k):
        v = below(draw(key, j), m - j)
        chosen = np.sort(idx[:, :j], axis=1)
        for i in range(j):
            v = v + (v >= chosen[:, i])
        idx[:, j] = v
    return idx


def relative_rotation(Rlo, Rhi):
    Rlo, Rhi = np.asarray(Rlo, np.float64).reshape(3, 3), np.asarray(Rhi, np.float64).reshape(3, 3)
    return np.array([[(Rhi[i, 0] * Rlo[j, 0] + Rhi[i, 1] * Rlo[j, 1]) + Rhi[i, 2] * Rlo[j, 2] for j in range(3)] for i in range(3)])


def points(xy, a, b, matches):
    """[m, 4] = (x_lo, y_lo, x_hi, y_hi) of the matches of the pair (a, b), either orientation"""
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    la, lb = (matches[:, 0], matches[:, 1]) if a < b else (matches[:, 1], matches[:, 0])
    return np.concatenate([xy[min(a, b)][la], xy[max(a, b)][lb]], 1).reshape(-1, 4)


def unit(E):
    """rows of E [H, 9] to unit norm, the squares summed left to right; (E, ok)"""
    with np.errstate(all="ignore"):
        n2 = E[:, 0] * E[:, 0]
        for k in range(1, 9):
            n2 = n2 + E[:, k] * E[:, k]
        n = np.sqrt(n2)
        ok = (n > 0) & np.isfinite(n)
        return E / n[:, None], ok


def eight_point(S):
    """S [H, 8, 4] -> (E [H, 9], valid [H]): verify_eight_row + verify_eight_solve for every hypothesis at once"""
    H = len(S)
    xl, yl, xh, yh = (S[:, :, k] for k in range(4))
    bad = np.isnan(S).any(axis=(1, 2))
    A = np.stack([xh * xl, xh * yl, xh, yh * xl, yh * yl, yh, xl, yl, np.ones_like(xl)], -1)
    A[bad] = 0.0
    scale = np.abs(A).reshape(H, 72).max(axis=1)
    perm = np.tile(np.arange(9), (H, 1))
    valid = ~bad
    ar = np.arange(H)
    with np.errstate(all="ignore"):
        for s in range(8):
            flat = np.abs(A[:, s:, s:]).reshape(H, -1)
            k = flat.argmax(axis=1)                   # the first of equals: the lowest (row, column)
            valid &= flat[ar, k] > PIVOT_REL * scale
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
        E, ok = unit(E)
    valid &= ok
    E[~valid] = 0.0
    return E, valid


def constraint(R, P):
    """c [n, 3] = x^_hi x (R x^_lo)"""
    xl, yl, xh, yh = (P[..., k] for k in range(4))
    q0 = (R[0, 0] * xl + R[0, 1] * yl) + R[0, 2]
    q1 = (R[1, 0] * xl + R[1, 1] * yl) + R[1, 2]
    q2 = (R[2, 0] * xl + R[2, 1] * yl) + R[2, 2]
    return np.stack([yh * q2 - q1, q0 - xh * q2, xh * q1 - yh * q0], -1)


def essential_from(t, R):
    """[t]x R for t [H, 3], unit norm; (E, ok)"""
    E = np.zeros((len(t), 9))
    for j in range(3):
        E[:, j] = t[:, 1] * R[2, j] - t[:, 2] * R[1, j]
        E[:, 3 + j] = t[:, 2] * R[0, j] - t[:, 0] * R[2, j]
        E[:, 6 + j] = t[:, 0] * R[1, j] - t[:, 1] * R[0, j]
    return unit(E)


def known_rotation(S, R):
    """S [H, 2, 4] -> (E [H, 9], valid [H])"""
    with np.errstate(all="ignore"):
        c1, c2 = constraint(R, S[:, 0]), constraint(R, S[:, 1])
        t = np.stack([c1[:, 1] * c2[:, 2] - c1[:, 2] * c2[:, 1], c1[:, 2] * c2[:, 0] - c1[:, 0] * c2[:, 2],
                      c1[:, 0] * c2[:, 1] - c1[:, 1] * c2[:, 0]], 1)
        tt = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
        n1 = (c1[:, 0] * c1[:, 0] + c1[:, 1] * c1[:, 1]) + c1[:, 2] * c1[:, 2]
        n2 = (c2[:, 0] * c2[:, 0] + c2[:, 1] * c2[:, 1]) + c2[:, 2] * c2[:, 2]
        valid = tt > T_REL2 * (n1 * n2)
        E, ok = essential_from(t, R)
    valid &= ok
    E[~valid] = 0.0
    return E, valid


def gate_terms(E, P):
    """(e^2, n_lo + n_hi) [H, m] of every (hypothesis, match): match_line_lo, match_norm_hi, match_gate"""
    E = np.asarray(E, np.float64).reshape(-1, 9)
    with np.errstate(invalid="ignore", over="ignore"):
        xl, yl, xh, yh = (P[None, :, k] for k in range(4))
        e = [E[:, k][:, None] for k in range(9)]
        l0 = (e[0] * xl + e[1] * yl) + e[2]
        l1 = (e[3] * xl + e[4] * yl) + e[5]
        l2 = (e[6] * xl + e[7] * yl) + e[8]
        n_lo = l0 * l0 + l1 * l1
        m0 = (e[0] * xh + e[3] * yh) + e[6]
        m1 = (e[1] * xh + e[4] * yh) + e[7]
        n_hi = m0 * m0 + m1 * m1
        r = (xh * l0 + yh * l1) + l2
        return r * r, n_lo + n_hi


def score(E, P, tau2, with_margin=False):
    """bool [H, m] (or [m] for one E): the inlier test"""
    e2, n = gate_terms(E, P)
    with np.errstate(invalid="ignore", over="ignore"):
        bound = tau2 * n
        ok = e2 <= bound
    if np.ndim(E) == 1 or np.shape(E) == (3, 3):
        ok, e2, bound = ok[0], e2[0], bound[0]
    if not with_margin:
        return ok
    fin = np.isfinite(e2) & np.isfinite(bound) & (bound > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(fin, np.abs(e2 - bound) / np.where(fin, bound, 1.0), np.inf)
    return ok, rel


def hypotheses(P, lo, hi, R=None, with_margin=False, **kw):
    """(E [H, 9], count [H], idx [H, k]) of every hypothesis of a pair with points P [m, 4]; invalid: E = 0, count = -1"""
    o = dict(DEFAULTS, **kw)
    H, k, m = int(o["hypotheses"]), sample_size(o["method"]), len(P)
    if m < k:
        out = np.zeros((H, 9)), np.full(H, -1, np.int64), np.zeros((H, k), np.int64)
        return out + (np.inf,) if with_margin else out
    idx = sample(o["seed"], lo, hi, H, m, k)
    S = P[idx]
    E, valid = eight_point(S) if o["method"] == EIGHT_POINT else known_rotation(S, np.asarray(R, np.float64).reshape(3, 3))
    tau2 = mo.tau2(o["intr"], o["max_error_px"])
    count = np.full(H, -1, np.int64)
    margin = np.inf
    step = max(1, (1 << 22) // max(m, 1))
    for h0 in range(0, H, step):
        res = score(E[h0:h0 + step], P, tau2, with_margin)
        ok = res[0] if with_margin else res
        if with_margin and valid[h0:h0 + step].any():
            margin = min(margin, res[1][valid[h0:h0 + step]].min(initial=np.inf))
        count[h0:h0 + step] = ok.sum(axis=1)
    count[~valid] = -1
    return (E, count, idx, margin) if with_margin else (E, count, idx)


def pick(count):
    """(best_h, count) of the winner: the highest count, the lowest h; (-1, -1) when every hypothesis is invalid"""
    h = int(np.argmax(count))
    return (h, int(count[h])) if count[h] >= 0 else (-1, -1)


def difference(E, F):
    """the largest entry of E - F with the sign of F fixed to E's (an essential matrix is defined up to sign); both unit norm"""
    E, F = np.asarray(E, np.float64).reshape(9), np.asarray(F, np.float64).reshape(9)
    return float(np.abs(E - (F if E @ F >= 0 else -F)).max())


def refit(E, P, tau2, method, R=None):
    """the refit of E over its inliers with LAPACK; None where there is none"""
    inl = score(E, P, tau2)
    Q = P[inl]
    if not len(Q):
        return None
    if method == EIGHT_POINT:
        xl, yl, xh, yh = (Q[:, k] for k in range(4))
        A = np.stack([xh * xl, xh * yl, xh, yh * xl, yh * yl, yh, xl, yl, np.ones_like(xl)], 1)
        w, v = np.linalg.eigh(A.T @ A)
        Uu, s, Vt = np.linalg.svd(v[:, 0].reshape(3, 3))
        if not s[1] > 0:
            return None
        F = (Uu @ np.diag([1.0, 1.0, 0.0]) @ Vt).reshape(9)
    else:
        c = constraint(np.asarray(R).reshape(3, 3), Q)
        w, v = np.linalg.eigh(c.T @ c)
        F = essential_from(v[:, 0][None, :], np.asarray(R).reshape(3, 3))[0][0]
    n = np.linalg.norm(F)
    return F / n if n > 0 and np.isfinite(n) else None


def verify_pair(P, lo, hi, R=None, **kw):
    """dict(E [9], status, n_inliers, best_h, mask [m]) of one pair; mask is all False unless the status is OK"""
    o = dict(DEFAULTS, **kw)
    m, k = len(P), sample_size(o["method"])
    out = dict(E=np.zeros(9), status=TOO_FEW_MATCHES, n_inliers=0, best_h=-1, mask=np.zeros(m, bool))
    if m < max(k, o["min_inliers"]):
        return out
    E, count, _ = hypotheses(P, lo, hi, R, **o)
    h, c = pick(count)
    if h < 0:
        out["status"] = NO_MODEL
        return out
    tau2 = mo.tau2(o["intr"], o["max_error_px"])
    best = E[h]
    for _ in range(int(o["refine_rounds"])):
        if c <= 0:
            break
        F = refit(best, P, tau2, o["method"], R)
        if F is None:
            break
        cn = int(score(F, P, tau2).sum())
        if cn <= c:
            break
        best, c = F, cn
    out.update(E=best, n_inliers=c, best_h=h, status=OK if c >= o["min_inliers"] else TOO_FEW_INLIERS)
    if out["status"] == OK:
        out["mask"] = score(best, P, tau2)
    return out
