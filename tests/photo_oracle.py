"""numpy restatement of the multi-view colour fusion (include/lvba_hip.h, "multi-view colour fusion and photometric consistency";
DESIGN.md §10p).

The rule, once more.  Point X = (double) of the floats, never sampled when a coordinate is not finite.  In image j: the fate of
the co-visibility stage (covis_oracle: behind, outside [0, W - 1) x [0, H - 1), hidden iff the float fetch of depth image j
succeeds with d and Z > d (1 + occlusion_rel) + occlusion_abs, a hole iff the fetch fails); sampled iff seen, or a hole with
holes != 0, and Z <= max_depth where max_depth > 0.  x = floor(u), a = floor((u - x) 256), likewise y, b; the four texels weigh
(256 - a)(256 - b), a (256 - b), (256 - a) b, a b; per channel c = sum weight byte, c16 = (c + 128) >> 8.  Per point n_views,
S1 = sum c16, S2 = sum c16^2 (channels b, g, r).  rgb = (2 S1 + 256 n) // (512 n) written r g b, sigma = sqrt(((N_b + N_g) + N_r)
/ (3 * 65536 * n n)) with N_c = n S2_c - S1_c^2, NaN below min_views.

The vectorised functions and the plain loops at the end (tiny cases only) are written independently of one another."""
import math

import numpy as np

import covis_oracle as co
import match_depth_oracle as mdo

F = np.float32
DEFAULTS = dict(occlusion_rel=0.05, occlusion_abs=0.1, max_depth=0.0, holes=0, min_views=2, max_batch_images=0)


def sample_image(X, image, depth, intr, R, t, **kw):
    """One image: (sampled bool [n], c16 int64 [n, 3] (b, g, r; 0 where not sampled), margins dict).  X float64 [n, 3]; image uint8
    [H, W, 3]; depth float32 [H, W] or None.  margins: `compare`, the smallest relative distance of an evaluated comparison from its
    bound (in-image, Z against the occlusion bound, Z against max_depth), and `texel`, the smallest distance in pixels of a sampled
    u or v from a multiple of 1/256."""
    o = dict(DEFAULTS, **kw)
    H, W = image.shape[:2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(X).all(1)
        u, v, Z, ok = co.project(intr, R, t, X)
        ok = ok & finite
        inside = (u >= 0.0) & (u < float(W - 1)) & (v >= 0.0) & (v < float(H - 1))
        compare = np.inf
        if ok.any():
            compare = min(np.min(np.minimum(np.abs(u[ok]), np.abs(u[ok] - (W - 1))) / (W - 1)),
                          np.min(np.minimum(np.abs(v[ok]), np.abs(v[ok] - (H - 1))) / (H - 1)))
        seen = ok & inside
        if depth is not None:
            d, got = co.fetch(np.asarray(depth, F)[None], 0, np.where(seen, u, np.nan).astype(F), np.where(seen, v, np.nan).astype(F))
            bound = d.astype(np.float64) * (1.0 + o["occlusion_rel"]) + o["occlusion_abs"]
            judged = seen & got
            if judged.any():
                compare = min(compare, np.min(np.abs(Z[judged] - bound[judged]) / bound[judged]))
            hidden = judged & (Z > bound)
            hole = seen & ~got
            seen = seen & ~hidden & (~hole | bool(o["holes"]))
        if o["max_depth"] > 0.0:
            if seen.any():
                compare = min(compare, np.min(np.abs(Z[seen] - o["max_depth"]) / o["max_depth"]))
            seen = seen & (Z <= o["max_depth"])
        us, vs = np.where(seen, u, 0.0), np.where(seen, v, 0.0)
        xf, yf = np.floor(us), np.floor(vs)
        a, b = np.floor((us - xf) * 256.0).astype(np.int64), np.floor((vs - yf) * 256.0).astype(np.int64)
        x, y = xf.astype(np.int64), yf.astype(np.int64)
        texel = np.inf
        if seen.any():
            for q in (us[seen], vs[seen]):
                s = q * 256.0
                texel = min(texel, np.min(np.abs(s - np.round(s))) / 256.0)
        img = image.astype(np.int64)
        c = ((256 - a) * (256 - b))[:, None] * img[y, x] + (a * (256 - b))[:, None] * img[y, np.minimum(x + 1, W - 1)] + \
            ((256 - a) * b)[:, None] * img[np.minimum(y + 1, H - 1), x] + (a * b)[:, None] * img[np.minimum(y + 1, H - 1), np.minimum(x + 1, W - 1)]
        c16 = np.where(seen[:, None], (c + 128) >> 8, 0)
    return seen, c16, dict(compare=float(compare), texel=float(texel))


def sums(points, images, depth, intr, Rcw, tcw, which=None, **kw):
    """(n_views int32 [n], S1 uint32 [n, 3], S2 int64 [n, 3], seen bool [M, n], margins) over the images `which` (default: all).
    points float32 [n, 3]; images uint8 [M, H, W, 3]; depth float32 [M, H, W] or None."""
    X = np.asarray(points, F).astype(np.float64).reshape(-1, 3)
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    n = len(X)
    nv, S1, S2 = np.zeros(n, np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    seen = np.zeros((len(images), n), bool)
    margins = dict(compare=np.inf, texel=np.inf)
    for j in (range(len(images)) if which is None else which):
        seen[j], c16, m = sample_image(X, images[j], None if depth is None else depth[j], intr, R[j], t[j], **kw)
        nv += seen[j]
        S1 += c16
        S2 += c16 * c16
        margins = {k: min(margins[k], m[k]) for k in margins}
    assert S1.max(initial=0) < 2 ** 32
    return nv.astype(np.int32), S1.astype(np.uint32), S2, seen, margins


def finish(nv, S1, S2, **kw):
    """(rgb uint8 [n, 3], sigma float64 [n])"""
    o = dict(DEFAULTS, **kw)
    n = np.asarray(nv, np.int64)
    S1, S2 = np.asarray(S1).astype(np.int64), np.asarray(S2, np.int64)
    nn = np.maximum(n, 1)[:, None]
    rgb = np.where(n[:, None] > 0, (2 * S1 + 256 * nn) // (512 * nn), 0)[:, ::-1].astype(np.uint8)
    N = n[:, None] * S2 - S1 * S1
    assert (N >= 0).all()
    Nd = N.astype(np.float64)
    with np.errstate(all="ignore"):
        sigma = np.sqrt(((Nd[:, 0] + Nd[:, 1]) + Nd[:, 2]) / (3.0 * 65536.0 * (n * n).astype(np.float64)))
    return np.ascontiguousarray(rgb), np.where(n >= o["min_views"], sigma, np.nan)


def summary(nv, sigma, **kw):
    """the summary's integers, mean_sigma as math.fsum over the valid points / n_valid, mean_views"""
    o = dict(DEFAULTS, **kw)
    n = np.asarray(nv, np.int64)
    valid = n >= o["min_views"]
    n_seen, n_valid, n_samples = int((n >= 1).sum()), int(valid.sum()), int(n.sum())
    return dict(n_points=len(n), n_seen=n_seen, n_valid=n_valid, n_samples=n_samples,
                mean_sigma=math.fsum(sigma[valid].tolist()) / n_valid if n_valid else math.nan,
                mean_views=n_samples / n_seen if n_seen else math.nan)


def evaluate(points, images, depth, intr, Rcw, tcw, **kw):
    """the whole rule: dict(n_views, s1, s2, rgb, sigma, summary, seen, margins)"""
    nv, S1, S2, seen, margins = sums(points, images, depth, intr, Rcw, tcw, **kw)
    rgb, sigma = finish(nv, S1, S2, **kw)
    return dict(n_views=nv, s1=S1, s2=S2, rgb=rgb, sigma=sigma, summary=summary(nv, sigma, **kw), seen=seen, margins=margins)


# ---- the rule as plain loops (tiny cases only), on the scalar functions of the matcher's oracles and Python integers
def loops_sums(points, images, depth, intr, Rcw, tcw, **kw):
    o = dict(DEFAULTS, **kw)
    M, H, W = images.shape[:3]
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    out = []
    with np.errstate(all="ignore"):
        for p in np.asarray(points, F).reshape(-1, 3):
            X = [float(p[0]), float(p[1]), float(p[2])]
            n, s1, s2 = 0, [0, 0, 0], [0, 0, 0]
            for j in range(M):
                if not all(math.isfinite(c) for c in X):
                    continue
                uv = mdo.project(intr, R[j], t[j], np.array(X))
                if uv is None or not (0.0 <= uv[0] < W - 1 and 0.0 <= uv[1] < H - 1):
                    continue
                Rj, tj = R[j], t[j]
                Z = float(Rj[2, 0]) * X[0] + float(Rj[2, 1]) * X[1] + float(Rj[2, 2]) * X[2] + float(tj[2])
                if depth is not None:
                    d = mdo.fetch_depth_bilinear(depth[j], F(uv[0]), F(uv[1]))
                    if d is None:
                        if not o["holes"]:
                            continue
                    elif Z > float(d) * (1.0 + o["occlusion_rel"]) + o["occlusion_abs"]:
                        continue
                if o["max_depth"] > 0.0 and not Z <= o["max_depth"]:
                    continue
                u, v = float(uv[0]), float(uv[1])
                x, y = int(math.floor(u)), int(math.floor(v))
                a, b = int(math.floor((u - x) * 256.0)), int(math.floor((v - y) * 256.0))
                n += 1
                for k in range(3):
                    c = (256 - a) * (256 - b) * int(images[j, y, x, k]) + a * (256 - b) * int(images[j, y, x + 1, k]) + \
                        (256 - a) * b * int(images[j, y + 1, x, k]) + a * b * int(images[j, y + 1, x + 1, k])
                    c16 = (c + 128) >> 8
                    s1[k] += c16
                    s2[k] += c16 * c16
            out.append((n, s1, s2))
    return out


def loops_finish(n, s1, s2, **kw):
    """(rgb [3] as r, g, b, sigma) of one point, on Python integers"""
    o = dict(DEFAULTS, **kw)
    rgb = [(2 * s1[k] + 256 * n) // (512 * n) if n > 0 else 0 for k in (2, 1, 0)]
    if n < o["min_views"]:
        return rgb, math.nan
    N = [n * s2[k] - s1[k] * s1[k] for k in range(3)]
    return rgb, math.sqrt(((float(N[0]) + float(N[1])) + float(N[2])) / (3.0 * 65536.0 * float(n * n)))
