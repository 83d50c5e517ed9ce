"""numpy restatement of the co-visibility pair selection (include/lvba_hip.h, "which image pairs to match").

The rule, once more.  Image i of W x H pixels gets G = grid_x grid_y cells, sample s = gy grid_x + gx, with the centre pixel
px = ((2 gx + 1)(W - 1)) // (2 grid_x), py likewise.  Candidates: the centre, then the Chebyshev rings r = 1 .. search_radius, each
walked dy = -r .. r and inside that dx = -r .. r keeping |dx| = r or |dy| = r; one outside [0, W - 2] x [0, H - 2] is skipped.  The
first candidate whose undistortion succeeds, that has a depth return (bilinear fetch in float arithmetic, all four neighbours
> 0) and whose world point R^T (x d, y d, d) - R^T t is finite is the cell's sample; a cell without one has no point (NaN).
Sample s of i is seen in j != i iff it has a point, projects under (R_j, t_j), lands in 0 <= u < W - 1, 0 <= v < H - 1 and -- with
occlusion on -- is not hidden: hidden iff the fetch of depth image j at the float pixel succeeds with d and
Z > d (1 + occlusion_rel) + occlusion_abs.  c_ij counts them, n_i the cells with a point, r_ij = c_ij / n_i.  For i < j the score is
max(r_ij, r_ji) and shared = max(c_ij, c_ji) (min with both_ways); eligible iff shared >= min_shared and score >= min_overlap; with
max_per_image = K > 0 an eligible pair is kept iff it is among the K best partners (score descending, index ascending) of i or of j.

Every expression in the header's order, one rounding per operation; the vectorised functions and the plain loops at the end
(tiny cases only) are written independently of one another."""
import numpy as np

import match_depth_oracle as mdo
import match_oracle as mo

F = np.float32
DEFAULTS = dict(grid_x=16, grid_y=12, search_radius=4, occlusion=1, both_ways=0, max_per_image=0, min_shared=8, min_overlap=0.1,
                occlusion_rel=0.05, occlusion_abs=0.1)
NO_POINT, BEHIND, OUTSIDE, HIDDEN, SEEN_HOLE, SEEN = range(6)


def centre(g, cells, size):
    return ((2 * g + 1) * (size - 1)) // (2 * cells)


def ring_offsets(radius):
    """[(dx, dy, r)] in the order the search visits them"""
    out = [(0, 0, 0)]
    for r in range(1, radius + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if abs(dx) == r or abs(dy) == r:
                    out.append((dx, dy, r))
    return out


def undistort(intr, u, v):
    """trk_undistort on fp64 arrays: (x, y, ok)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    ok = np.isfinite(u) & np.isfinite(v)
    if abs(fx) < 1e-12 or abs(fy) < 1e-12:
        ok = np.zeros_like(ok)
    xd, yd = (u - cx) / fx, (v - cy) / fy
    xu, yu = xd, yd
    for _ in range(8):
        r2 = xu * xu + yu * yu
        r4 = r2 * r2
        radial = 1.0 + k1 * r2 + k2 * r4
        ok = ok & ~(np.abs(radial) < 1e-12) & np.isfinite(radial)
        xt = 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu)
        yt = p1 * (r2 + 2.0 * yu * yu) + 2.0 * p2 * xu * yu
        xu, yu = (xd - xt) / radial, (yd - yt) / radial
        ok = ok & np.isfinite(xu) & np.isfinite(yu)
    return xu, yu, ok


def fetch(depth, m, u, v):
    """fetchDepthBilinear of images depth[m] at the float32 pixels (u, v): (d float32, ok)"""
    _, h, w = depth.shape
    u, v = np.asarray(u, F), np.asarray(v, F)
    ok = np.isfinite(u) & np.isfinite(v) & ~((u < 0) | (v < 0) | (u >= F(w - 1)) | (v >= F(h - 1)))
    x, y = np.where(ok, np.floor(u), 0).astype(np.int64), np.where(ok, np.floor(v), 0).astype(np.int64)
    du, dv = u - x.astype(F), v - y.astype(F)
    d00, d10, d01, d11 = depth[m, y, x], depth[m, y, x + 1], depth[m, y + 1, x], depth[m, y + 1, x + 1]
    ok = ok & ~((d00 <= 0) | (d10 <= 0) | (d01 <= 0) | (d11 <= 0))
    one = F(1)
    d = ((one - du) * (one - dv)) * d00
    d = d + ((du * (one - dv)) * d10)
    d = d + (((one - du) * dv) * d01)
    d = d + ((du * dv) * d11)
    assert d.dtype == F
    return d, ok & (d > 0)


def samples(depth, intr, Rcw, tcw, **kw):
    """(world [M, G, 3] with NaN rows, ring [M, G]: the ring a cell was resolved on, -1 for none)"""
    o = dict(DEFAULTS, **kw)
    depth = np.asarray(depth, F)
    M, H, W = depth.shape
    gx_n, gy_n = o["grid_x"], o["grid_y"]
    G = gx_n * gy_n
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3)[:M], np.asarray(tcw, np.float64).reshape(-1, 3)[:M]
    s = np.arange(G)
    px, py = centre(s % gx_n, gx_n, W), centre(s // gx_n, gy_n, H)
    img = np.repeat(np.arange(M), G)
    px, py = np.tile(px, M), np.tile(py, M)
    world, ring = np.full((M * G, 3), np.nan), np.full(M * G, -1)
    with np.errstate(all="ignore"):
        for dx, dy, r in ring_offsets(o["search_radius"]):
            todo = np.flatnonzero(ring < 0)
            u, v = px[todo] + dx, py[todo] + dy
            inside = (u >= 0) & (v >= 0) & (u <= W - 2) & (v <= H - 2)
            todo, u, v = todo[inside], u[inside], v[inside]
            if not len(todo):
                continue
            m = img[todo]
            uf, vf = u.astype(F), v.astype(F)
            x, y, ok = undistort(intr, uf.astype(np.float64), vf.astype(np.float64))
            d, has = fetch(depth, m, uf, vf)
            dd = d.astype(np.float64)
            Xc = [x * dd, y * dd, dd]
            ok = ok & has & np.isfinite(Xc[0]) & np.isfinite(Xc[1]) & np.isfinite(Xc[2])
            Rm, tm = R[m], t[m]
            p = []
            for k in range(3):
                twc = -(Rm[:, 0, k] * tm[:, 0] + Rm[:, 1, k] * tm[:, 1] + Rm[:, 2, k] * tm[:, 2])
                p.append((Rm[:, 0, k] * Xc[0] + Rm[:, 1, k] * Xc[1] + Rm[:, 2, k] * Xc[2]) + twc)
            p = np.stack(p, 1)
            ok = ok & np.isfinite(p).all(1)
            world[todo[ok]] = p[ok]
            ring[todo[ok]] = r
    return world.reshape(M, G, 3), ring.reshape(M, G)


def project(intr, R, t, X):
    """trk_project of points X [n, 3] under one pose: (u, v, Z, ok)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    X0 = R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]
    X1 = R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]
    Z = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
    ok = np.isfinite(X0) & np.isfinite(X1) & np.isfinite(Z) & ~(Z <= 1e-12)
    x, y = X0 / Z, X1 / Z
    r2 = x * x + y * y
    r4 = r2 * r2
    radial = 1.0 + k1 * r2 + k2 * r4
    xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
    yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
    ok = ok & np.isfinite(xd) & np.isfinite(yd)
    u, v = fx * xd + cx, fy * yd + cy
    return u, v, Z, ok & np.isfinite(u) & np.isfinite(v)


def fates(depth, intr, Rcw, tcw, world, with_margin=False, **kw):
    """int [M, M, G]: what becomes of sample s of image i in image j (the diagonal is NO_POINT); with_margin: also the smallest
    distance of an evaluated comparison from its bound -- the in-image ones relative to the image size, Z relative to its bound"""
    o = dict(DEFAULTS, **kw)
    depth = np.asarray(depth, F)
    M, H, W = depth.shape
    G = world.shape[1]
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    X = world.reshape(M * G, 3)
    has = ~np.isnan(X[:, 0])
    out = np.zeros((M, M, G), np.int64)
    margin = np.inf
    with np.errstate(all="ignore"):
        for j in range(M):
            u, v, Z, ok = project(intr, R[j], t[j], X)
            inside = (u >= 0.0) & (u < float(W - 1)) & (v >= 0.0) & (v < float(H - 1))
            f = np.where(ok, np.where(inside, SEEN, OUTSIDE), BEHIND)
            ev = has & ok
            ev[j * G:(j + 1) * G] = False
            if ev.any():
                margin = min(margin, np.min(np.minimum(np.abs(u[ev]), np.abs(u[ev] - (W - 1))) / (W - 1)),
                             np.min(np.minimum(np.abs(v[ev]), np.abs(v[ev] - (H - 1))) / (H - 1)))
            if o["occlusion"]:
                d, got = fetch(depth, j, np.where(ok, u, np.nan).astype(F), np.where(ok, v, np.nan).astype(F))
                bound = d.astype(np.float64) * (1.0 + o["occlusion_rel"]) + o["occlusion_abs"]
                vis = f == SEEN
                f = np.where(vis & ~got, SEEN_HOLE, np.where(vis & (Z > bound), HIDDEN, f))
                ev = ev & vis & got
                if ev.any():
                    margin = min(margin, np.min(np.abs(Z[ev] - bound[ev]) / bound[ev]))
            f = np.where(has, f, NO_POINT)
            out[:, j] = f.reshape(M, G)
            out[j, j] = NO_POINT
    return (out, margin) if with_margin else out


def counts(fate, world):
    """(n_points [M], counts [M, M]) int32"""
    return (~np.isnan(world[:, :, 0])).sum(1).astype(np.int32), (fate >= SEEN_HOLE).sum(2).astype(np.int32)


def pair_terms(n, c, **kw):
    """(score [M, M], shared [M, M], eligible [M, M]), symmetric, the diagonal not eligible"""
    o = dict(DEFAULTS, **kw)
    n, c = np.asarray(n, np.int64), np.asarray(c, np.int64)
    with np.errstate(all="ignore"):
        r = np.where(n[:, None] > 0, c.astype(np.float64) / n[:, None].astype(np.float64), 0.0)
    if o["both_ways"]:
        score, shared = np.minimum(r, r.T), np.minimum(c, c.T)
    else:
        score, shared = np.maximum(r, r.T), np.maximum(c, c.T)
    eligible = (shared >= o["min_shared"]) & (score >= o["min_overlap"])
    np.fill_diagonal(eligible, False)
    return score, shared, eligible


def ranked_partners(score, eligible, i):
    """the eligible partners of image i, best first: score descending, index ascending"""
    p = np.flatnonzero(eligible[i])
    return p[np.lexsort((p, -score[i, p]))]


def select(n, c, **kw):
    """(pairs [m, 2] int32 sorted by (i, j), score [m], shared [m, 2] int32 = (c_ij, c_ji))"""
    o = dict(DEFAULTS, **kw)
    score, _, eligible = pair_terms(n, c, **o)
    keep = eligible.copy()
    K = o["max_per_image"]
    if K > 0:
        top = np.zeros_like(eligible)
        for i in range(len(score)):
            top[i, ranked_partners(score, eligible, i)[:K]] = True
        keep = eligible & (top | top.T)
    i, j = np.nonzero(np.triu(keep, 1))
    c = np.asarray(c, np.int32)
    return np.stack([i, j], 1).astype(np.int32), score[i, j], np.stack([c[i, j], c[j, i]], 1).astype(np.int32)


def select_pairs(depth, intr, Rcw, tcw, **kw):
    """the whole call: (pairs, score, shared, n_points)"""
    world, _ = samples(depth, intr, Rcw, tcw, **kw)
    n, c = counts(fates(depth, intr, Rcw, tcw, world, **kw), world)
    return select(n, c, **kw) + (n,)


# ---- the rule as plain loops (tiny cases only), on the scalar functions of the matcher's oracles
def loops_samples(depth, intr, Rcw, tcw, **kw):
    o = dict(DEFAULTS, **kw)
    M, H, W = depth.shape
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    world = np.full((M, o["grid_x"] * o["grid_y"], 3), np.nan)
    with np.errstate(all="ignore"):
        for i in range(M):
            for gy in range(o["grid_y"]):
                for gx in range(o["grid_x"]):
                    px, py = centre(gx, o["grid_x"], W), centre(gy, o["grid_y"], H)
                    for dx, dy, _ in ring_offsets(o["search_radius"]):
                        u, v = px + dx, py + dy
                        if u < 0 or v < 0 or u > W - 2 or v > H - 2:
                            continue
                        xy = mo.undistort(intr, float(F(u)), float(F(v)))
                        if xy is None:
                            continue
                        p = mdo.lift(depth[i], F(u), F(v), xy, R[i], t[i])
                        if p is not None:
                            world[i, gy * o["grid_x"] + gx] = p
                            break
    return world


def loops_counts(depth, intr, Rcw, tcw, world, **kw):
    o = dict(DEFAULTS, **kw)
    M, H, W = depth.shape
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    n, c = np.zeros(M, np.int32), np.zeros((M, M), np.int32)
    with np.errstate(all="ignore"):
        for i in range(M):
            for X in world[i]:
                if np.isnan(X[0]):
                    continue
                n[i] += 1
                for j in range(M):
                    if j == i:
                        continue
                    uv = mdo.project(intr, R[j], t[j], X)
                    if uv is None or not (0.0 <= uv[0] < W - 1 and 0.0 <= uv[1] < H - 1):
                        continue
                    if o["occlusion"]:
                        d = mdo.fetch_depth_bilinear(depth[j], F(uv[0]), F(uv[1]))
                        if d is not None:
                            Rj, tj = R[j], t[j]
                            Z = float(Rj[2, 0]) * float(X[0]) + float(Rj[2, 1]) * float(X[1]) + float(Rj[2, 2]) * float(X[2]) + float(tj[2])
                            if Z > float(d) * (1.0 + o["occlusion_rel"]) + o["occlusion_abs"]:
                                continue
                    c[i, j] += 1
    return n, c


def loops_select(n, c, **kw):
    o = dict(DEFAULTS, **kw)
    M, K = len(n), o["max_per_image"]

    def terms(i, j):
        rij = float(c[i][j]) / float(n[i]) if n[i] > 0 else 0.0
        rji = float(c[j][i]) / float(n[j]) if n[j] > 0 else 0.0
        pick = min if o["both_ways"] else max
        score, shared = pick(rij, rji), pick(int(c[i][j]), int(c[j][i]))
        return score, shared >= o["min_shared"] and score >= o["min_overlap"]

    def rank(i, j):
        """how many eligible partners of i come before j"""
        sj = terms(i, j)[0]
        before = 0
        for p in range(M):
            if p in (i, j):
                continue
            sp, ok = terms(i, p)
            if ok and (sp > sj or (sp == sj and p < j)):
                before += 1
        return before

    out = []
    for i in range(M):
        for j in range(i + 1, M):
            score, ok = terms(i, j)
            if ok and (K == 0 or rank(i, j) < K or rank(j, i) < K):
                out.append((i, j, score, int(c[i][j]), int(c[j][i])))
    return out
