"""numpy restatement of the descriptor matcher (include/lvba_hip.h, "descriptor matching of image pairs"): int64 scores, the rules
literally, the gate in fp64 in the header's expression order.  This is the project's own definition of SiftMatchGPU's three
documented parameters; it is not pinned against SiftGPU."""
import numpy as np

DEFAULTS = dict(max_distance=0.7, max_ratio=0.8, mutual=1, guided=0, max_epipolar_px=4.0)
BASELINE_REL2 = 1e-20


def scores(A, B):
    return A.astype(np.int64) @ B.astype(np.int64).T


def scores_biased(A, B):
    """the identity the kernel uses: signed bytes a' = a - 128"""
    Ab, Bb = A.astype(np.int64) - 128, B.astype(np.int64) - 128
    return Ab @ Bb.T + 128 * Ab.sum(1)[:, None] + 128 * Bb.sum(1)[None, :] + 128 * 128 * 128


def distance(s):
    return np.arccos(np.minimum(np.asarray(s, np.float64) / 262144.0, 1.0))


def undistort(intr, u, v):
    """trk_undistort of tracks_device.h, operation for operation"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    u, v = float(u), float(v)
    if not (np.isfinite(u) and np.isfinite(v)) or abs(fx) < 1e-12 or abs(fy) < 1e-12:
        return None
    xd, yd = (u - cx) / fx, (v - cy) / fy
    xu, yu = xd, yd
    for _ in range(8):
        r2 = xu * xu + yu * yu
        r4 = r2 * r2
        radial = 1.0 + k1 * r2 + k2 * r4
        if abs(radial) < 1e-12 or not np.isfinite(radial):
            return None
        xt = 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu)
        yt = p1 * (r2 + 2.0 * yu * yu) + 2.0 * p2 * xu * yu
        xu, yu = (xd - xt) / radial, (yd - yt) / radial
        if not (np.isfinite(xu) and np.isfinite(yu)):
            return None
    return xu, yu


def undistort_all(intr, uv):
    """[n, 2] fp64, NaN where the undistortion fails (uv are fp32 pixels)"""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    out = np.full((len(uv), 2), np.nan)
    with np.errstate(all="ignore"):
        for i, (u, v) in enumerate(uv):
            r = undistort(intr, u, v)
            if r is not None:
                out[i] = r
    return out


def essential(Rlo, tlo, Rhi, thi):
    """E of (lo, hi), every sum left to right; zero when the centres coincide"""
    Rlo, Rhi = np.asarray(Rlo, np.float64).reshape(3, 3), np.asarray(Rhi, np.float64).reshape(3, 3)
    tlo, thi = [float(x) for x in tlo], [float(x) for x in thi]
    R = [[(float(Rhi[i, 0]) * float(Rlo[j, 0]) + float(Rhi[i, 1]) * float(Rlo[j, 1])) + float(Rhi[i, 2]) * float(Rlo[j, 2])
          for j in range(3)] for i in range(3)]
    t = [thi[i] - ((R[i][0] * tlo[0] + R[i][1] * tlo[1]) + R[i][2] * tlo[2]) for i in range(3)]
    tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    ref = ((tlo[0] * tlo[0] + tlo[1] * tlo[1]) + tlo[2] * tlo[2]) + ((thi[0] * thi[0] + thi[1] * thi[1]) + thi[2] * thi[2])
    E = np.zeros((3, 3))
    if tt <= BASELINE_REL2 * ref:
        return E
    for j in range(3):
        E[0, j] = t[1] * R[2][j] - t[2] * R[1][j]
        E[1, j] = t[2] * R[0][j] - t[0] * R[2][j]
        E[2, j] = t[0] * R[1][j] - t[1] * R[0][j]
    return E


def gate_terms(E, xy_lo, xy_hi):
    """(e^2, bound / tau^2) [n_lo, n_hi] of every (keypoint of lo, keypoint of hi)"""
    with np.errstate(invalid="ignore"):
        x, y = xy_lo[:, 0], xy_lo[:, 1]
        l0 = (E[0, 0] * x + E[0, 1] * y) + E[0, 2]
        l1 = (E[1, 0] * x + E[1, 1] * y) + E[1, 2]
        l2 = (E[2, 0] * x + E[2, 1] * y) + E[2, 2]
        n_lo = l0 * l0 + l1 * l1
        hx, hy = xy_hi[:, 0], xy_hi[:, 1]
        m0 = (E[0, 0] * hx + E[1, 0] * hy) + E[2, 0]
        m1 = (E[0, 1] * hx + E[1, 1] * hy) + E[2, 1]
        n_hi = m0 * m0 + m1 * m1
        e = (hx[None, :] * l0[:, None] + hy[None, :] * l1[:, None]) + l2[:, None]
        return e * e, n_lo[:, None] + n_hi[None, :]


def tau2(intr, max_epipolar_px):
    tau = (2.0 * float(max_epipolar_px)) / (float(intr[0]) + float(intr[1]))
    return tau * tau


class Geometry:
    def __init__(self, keypoints, intr, Rcw, tcw):
        self.intr = np.asarray(intr, np.float64)
        self.xy = [undistort_all(self.intr, k) for k in keypoints]
        self.R = np.asarray(Rcw, np.float64).reshape(-1, 3, 3)
        self.t = np.asarray(tcw, np.float64).reshape(-1, 3)

    def mask(self, a, b, max_epipolar_px, with_margin=False):
        """bool [n_a, n_b]: which candidates of the ordered pair (a, b) pass the gate"""
        lo, hi = min(a, b), max(a, b)
        E = essential(self.R[lo], self.t[lo], self.R[hi], self.t[hi])
        e2, n = gate_terms(E, self.xy[lo], self.xy[hi])
        with np.errstate(invalid="ignore"):
            bound = tau2(self.intr, max_epipolar_px) * n
            ok = e2 <= bound                         # [n_lo, n_hi]; NaN -> False
        out = ok if a < b else ok.T
        if not with_margin:
            return out
        fin = np.isfinite(e2) & np.isfinite(bound) & (bound > 0)
        margin = np.min(np.abs(e2[fin] - bound[fin]) / bound[fin]) if fin.any() else np.inf
        return out, margin


def top_two(S, mask=None):
    """best, s1, s2 of every row of the score matrix S [n_a, n_b] over the columns that take part"""
    n_a, n_b = S.shape
    best = np.full(n_a, -1, np.int64)
    s1 = np.zeros(n_a, np.int64)
    s2 = np.zeros(n_a, np.int64)
    if n_b == 0:
        return best, s1, s2
    T = S.astype(np.int64).copy()
    if mask is not None:
        T[~mask] = -1
    b = np.argmax(T, axis=1)                       # the lowest column of a tie
    r = np.arange(n_a)
    has = T[r, b] >= 0
    best[has] = b[has]
    s1[has] = T[r, b][has]
    T[r, b] = -1
    if n_b > 1:
        s2 = np.maximum(T.max(axis=1), 0)
    s2[~has] = 0
    return best, s1, s2


def scan(descs, a, b, geom=None, **kw):
    o = dict(DEFAULTS, **kw)
    S = scores(descs[a], descs[b])
    mask = geom.mask(a, b, o["max_epipolar_px"]) if o["guided"] else None
    return top_two(S, mask)


def match_pair(descs, a, b, geom=None, **kw):
    """(matches int64 [m, 2] by ascending r, scores [m]) of the ordered pair (a, b)"""
    o = dict(DEFAULTS, **kw)
    best, s1, s2 = scan(descs, a, b, geom, **o)
    d1, d2 = distance(s1), distance(s2)
    ok = (best >= 0) & (d1 < o["max_distance"]) & (d1 < o["max_ratio"] * d2)
    if o["mutual"]:
        back, _, _ = scan(descs, b, a, geom, **o)
        if len(back):
            ok &= back[np.maximum(best, 0)] == np.arange(len(best))
    r = np.flatnonzero(ok)
    return np.stack([r, best[r]], 1).astype(np.int64), s1[r]


def match_pairs(descs, pairs, geom=None, **kw):
    """(matches [m, 2], scores [m], match_off [n_pairs + 1]) in the caller's pair order"""
    ms, ss, off = [], [], [0]
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        m, s = match_pair(descs, int(a), int(b), geom, **kw)
        ms.append(m); ss.append(s); off.append(off[-1] + len(m))
    if not ms:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.array(off, np.int64)
    return np.concatenate(ms), np.concatenate(ss), np.array(off, np.int64)


def brute_scan(A, B, mask=None):
    """the definition as three loops (tiny cases only)"""
    best, s1, s2 = [], [], []
    for r in range(len(A)):
        cand = [(sum(int(x) * int(y) for x, y in zip(A[r], B[c])), c) for c in range(len(B)) if mask is None or mask[r, c]]
        if not cand:
            best.append(-1); s1.append(0); s2.append(0)
            continue
        top = max(cand, key=lambda sc: (sc[0], -sc[1]))
        rest = [s for s, c in cand if c != top[1]]
        best.append(top[1]); s1.append(top[0]); s2.append(max(rest) if rest else 0)
    return np.array(best, np.int64), np.array(s1, np.int64), np.array(s2, np.int64)
