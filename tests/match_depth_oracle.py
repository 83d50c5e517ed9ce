"""numpy restatement of the descriptor matcher's depth-guided gate (include/lvba_hip.h, "Depth-guided gate").
Scores, top two, distances and the undistortion are tests/match_oracle.py's; this adds the lifting of a keypoint through its depth
image (float arithmetic of the fetch, fp64 after it), the prediction of a lifted point in another image, and the gate's mask --
every expression in the header's order, one rounding per operation."""
import numpy as np

import match_oracle as mo

DEFAULTS = dict(mo.DEFAULTS, max_reproj_px=8.0)
F = np.float32


def fetch_depth_bilinear(img, u, v):
    """fetchDepthBilinear on a float32 image [h, w] at the fp32 pixel (u, v): None without a return"""
    h, w = img.shape
    u, v = F(u), F(v)
    if not (np.isfinite(u) and np.isfinite(v)):
        return None
    if u < 0 or v < 0 or u >= F(w - 1) or v >= F(h - 1):
        return None
    x, y = int(np.floor(u)), int(np.floor(v))
    du, dv = F(u - F(x)), F(v - F(y))
    d00, d10, d01, d11 = F(img[y, x]), F(img[y, x + 1]), F(img[y + 1, x]), F(img[y + 1, x + 1])
    if d00 <= 0 or d10 <= 0 or d01 <= 0 or d11 <= 0:
        return None
    one = F(1)
    d = F(F(F(one - du) * F(one - dv)) * d00)
    d = F(d + F(F(du * F(one - dv)) * d10))
    d = F(d + F(F(F(one - du) * dv) * d01))
    d = F(d + F(F(du * dv) * d11))
    return d if d > 0 else None


def lift(img, u, v, xy, R, t):
    """the world point of a keypoint (fp32 pixel, its undistorted point xy), or None: X^c = (x d, y d, d), R^T X^c - R^T t"""
    d = fetch_depth_bilinear(img, u, v)
    if d is None or not np.isfinite(xy).all():
        return None
    dd = float(d)
    Xc = (float(xy[0]) * dd, float(xy[1]) * dd, dd)
    if not np.isfinite(Xc).all():
        return None
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    t = [float(x) for x in t]
    p = []
    for r in range(3):
        twc = -(R[0][r] * t[0] + R[1][r] * t[1] + R[2][r] * t[2])
        p.append((R[0][r] * Xc[0] + R[1][r] * Xc[1] + R[2][r] * Xc[2]) + twc)
    return p if np.isfinite(p).all() else None


def project(intr, R, t, X):
    """trk_project of tracks_device.h, operation for operation: the distorted pixel, or None (nowhere)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    t = [float(x) for x in t]
    X = [float(x) for x in X]
    X0 = R[0][0] * X[0] + R[0][1] * X[1] + R[0][2] * X[2] + t[0]
    X1 = R[1][0] * X[0] + R[1][1] * X[1] + R[1][2] * X[2] + t[1]
    Z = R[2][0] * X[0] + R[2][1] * X[1] + R[2][2] * X[2] + t[2]
    if not (np.isfinite(X0) and np.isfinite(X1) and np.isfinite(Z)) or Z <= 1e-12:
        return None
    x, y = X0 / Z, X1 / Z
    r2 = x * x + y * y
    r4 = r2 * r2
    radial = 1.0 + k1 * r2 + k2 * r4
    xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
    yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
    if not (np.isfinite(xd) and np.isfinite(yd)):
        return None
    u, v = fx * xd + cx, fy * yd + cy
    return (u, v) if np.isfinite(u) and np.isfinite(v) else None


class DepthGeometry(mo.Geometry):
    """mo.Geometry (the epipolar gate stays available) with the lifted points of every keypoint; depth [n_images, h, w] float32"""

    def __init__(self, keypoints, intr, Rcw, tcw, depth):
        super().__init__(keypoints, intr, Rcw, tcw)
        self.uv = [np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints]
        self.points = []
        with np.errstate(all="ignore"):
            for i, uv in enumerate(self.uv):
                P = np.full((len(uv), 3), np.nan)
                for k, (u, v) in enumerate(uv):
                    p = lift(depth[i], u, v, self.xy[i][k], self.R[i], self.t[i])
                    if p is not None:
                        P[k] = p
                self.points.append(P)
        self._pred = {}

    def predictions(self, a, b):
        """[n_a, 2]: the keypoints of a in image b; NaN rows have no point, +inf rows are nowhere"""
        if (a, b) not in self._pred:
            out = np.full((len(self.uv[a]), 2), np.nan)
            with np.errstate(all="ignore"):
                for k, X in enumerate(self.points[a]):
                    if not np.isnan(X[0]):
                        p = project(self.intr, self.R[b], self.t[b], X)
                        out[k] = p if p is not None else np.inf
            self._pred[(a, b)] = out
        return self._pred[(a, b)]

    def terms(self, a, b):
        """(hp [n_a], hq [n_b], d2(p -> q) [n_a, n_b], d2(q -> p) [n_a, n_b]) of the ordered pair (a, b)"""
        Pa, Pb = self.predictions(a, b), self.predictions(b, a)
        ua, ub = self.uv[a].astype(np.float64), self.uv[b].astype(np.float64)
        with np.errstate(all="ignore"):
            du, dv = ub[None, :, 0] - Pa[:, None, 0], ub[None, :, 1] - Pa[:, None, 1]
            d2_pq = du * du + dv * dv
            du, dv = ua[:, None, 0] - Pb[None, :, 0], ua[:, None, 1] - Pb[None, :, 1]
            d2_qp = du * du + dv * dv
        return ~np.isnan(Pa[:, 0]), ~np.isnan(Pb[:, 0]), d2_pq, d2_qp

    def depth_mask(self, a, b, max_reproj_px, with_margin=False):
        """bool [n_a, n_b]: which candidates of the ordered pair (a, b) pass the depth gate"""
        hp, hq, d2_pq, d2_qp = self.terms(a, b)
        rho2 = float(max_reproj_px) * float(max_reproj_px)
        with np.errstate(invalid="ignore"):
            near_q, near_p = d2_pq <= rho2, d2_qp <= rho2
        out = (hp[:, None] | hq[None, :]) & (near_q | ~hp[:, None]) & (near_p | ~hq[None, :])
        if not with_margin:
            return out
        # every evaluated distance that is a number: an infinite or NaN distance fails exactly
        ev = np.concatenate([d2_pq[hp][np.isfinite(d2_pq[hp])].ravel(), d2_qp[:, hq][np.isfinite(d2_qp[:, hq])].ravel()])
        return out, (np.min(np.abs(ev - rho2) / rho2) if len(ev) else np.inf)

    def branches(self, a, b):
        """how many candidates of (a, b) fall into each branch of the rule: (both have points, only the row, only the column, neither)"""
        hp, hq, _, _ = self.terms(a, b)
        n = lambda x, y: int(x.sum()) * int(y.sum())
        return n(hp, hq), n(hp, ~hq), n(~hp, hq), n(~hp, ~hq)


def loops_mask(g, a, b, max_reproj_px):
    """the rule as plain loops over the candidates (tiny cases only)"""
    rho2 = float(max_reproj_px) * float(max_reproj_px)
    out = np.zeros((len(g.uv[a]), len(g.uv[b])), bool)

    def near(X, j, q):
        pr = project(g.intr, g.R[j], g.t[j], X)
        if pr is None:
            return False
        du, dv = float(q[0]) - pr[0], float(q[1]) - pr[1]
        return du * du + dv * dv <= rho2                     # NaN: False

    with np.errstate(all="ignore"):
        for r in range(out.shape[0]):
            for c in range(out.shape[1]):
                Xp, Xq = g.points[a][r], g.points[b][c]
                hp, hq = not np.isnan(Xp[0]), not np.isnan(Xq[0])
                if not (hp or hq):
                    continue
                ok = True
                if hp:
                    ok = ok and near(Xp, b, g.uv[b][c])
                if hq:
                    ok = ok and near(Xq, a, g.uv[a][r])
                out[r, c] = ok
    return out


def scan(descs, a, b, geom=None, **kw):
    o = dict(DEFAULTS, **kw)
    mask = None
    if o["guided"] == 2:
        mask = geom.depth_mask(a, b, o["max_reproj_px"])
    elif o["guided"] == 1:
        mask = geom.mask(a, b, o["max_epipolar_px"])
    return mo.top_two(mo.scores(descs[a], descs[b]), mask)


def match_pair(descs, a, b, geom=None, **kw):
    """mo.match_pair with the three gates"""
    o = dict(DEFAULTS, **kw)
    best, s1, s2 = scan(descs, a, b, geom, **o)
    d1, d2 = mo.distance(s1), mo.distance(s2)
    ok = (best >= 0) & (d1 < o["max_distance"]) & (d1 < o["max_ratio"] * d2)
    if o["mutual"]:
        back, _, _ = scan(descs, b, a, geom, **o)
        if len(back):
            ok &= back[np.maximum(best, 0)] == np.arange(len(best))
    r = np.flatnonzero(ok)
    return np.stack([r, best[r]], 1).astype(np.int64), s1[r]


def match_pairs(descs, pairs, geom=None, **kw):
    ms, ss, off = [], [], [0]
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        m, s = match_pair(descs, int(a), int(b), geom, **kw)
        ms.append(m); ss.append(s); off.append(off[-1] + len(m))
    if not ms:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.array(off, np.int64)
    return np.concatenate(ms), np.concatenate(ss), np.array(off, np.int64)
