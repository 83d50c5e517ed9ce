"""Restatement of the per-image exposure compensation (include/lvba_hip.h, "per-image exposure compensation of the colour fusion";
DESIGN.md §10r) in numpy int64 and, where a product needs more than 64 bits, Python integers.

The rule, once more.  Gains (A, B) per image and channel (b, g, r), A in 2^-16, B in 2^-16 of 1/256 grey level, identity (65536, 0);
c' = clamp((A c16 + B + 32768) // 65536, 0, 65280).  The fusion with gains adds c' where the plain one adds c16.  Estimation sums per
image against ref16 / valid under gains_in: a valid point is located as the fusion locates it; channel k is used iff its four texel
bytes lie in [sat_lo, sat_hi] and, where gate > 0, |c' - ref| <= 256 gate; per channel n, sum c, sum ref, sum c^2, sum c ref,
sum (c' - ref)^2 (c raw), then n_located and the terms the gate refused.  Solve per channel: TOO_FEW below min_samples; affine with
D = n sum c^2 - (sum c)^2 <= n^2 (256 min_spread)^2 falls back to the gain-only form; A = (N 2^16 + D // 2) // D with
N = n sum c ref - sum c sum ref, B = ((sum ref 2^16 - A sum c) 2 + n) // (2 n); gain-only A = (sum c ref 2^16 + sum c^2 // 2) //
sum c^2, B = 0; OUT_OF_BOUNDS outside the gain and offset limits.  An image is the worst of its channels, identity on all three from
TOO_FEW on.  Gauge per channel over the OK and FALLBACK_GAIN images: S = (n_ok 2^32 + sum A // 2) // sum A, A <- (A S + 2^15) >> 16,
B <- ((B S + 2^15) >> 16) - T, T = (2 sum B + n_ok) // (2 n_ok); gauged gains the fusion would refuse make the image OUT_OF_BOUNDS.

The vectorised functions and the plain loops at the end (tiny cases only) are written independently of one another."""
import math

import numpy as np

import covis_oracle as co
import photo_oracle as po

DEFAULTS = dict(occlusion_rel=0.05, occlusion_abs=0.1, max_depth=0.0, min_gain=0.25, max_gain=4.0, max_offset=64.0, holes=0, model=0,
                sat_lo=4, sat_hi=251, gate=30, min_samples=200, min_spread=2, max_batch_images=0)
N_SUMS = 20
ONE = 65536
C_MAX = 65280
OK, FALLBACK_GAIN, TOO_FEW_SAMPLES, OUT_OF_BOUNDS = range(4)
AFFINE, GAIN = 0, 1
A_MIN, A_MAX, B_MAX = 1 << 14, 1 << 18, 65536 * 65280
LOCATE = ("occlusion_rel", "occlusion_abs", "max_depth", "holes")


def identity(m):
    g = np.zeros((m, 3, 2), np.int64)
    g[:, :, 0] = ONE
    return g


def apply(A, B, c16):
    """c' of c16 (int64 arrays or scalars): numpy's // floors"""
    return np.clip((np.asarray(A, np.int64) * np.asarray(c16, np.int64) + B + 32768) // ONE, 0, C_MAX)


def locate_opts(kw):
    return {k: v for k, v in kw.items() if k in LOCATE}


def taps(X, image, depth, intr, R, t, **kw):
    """(sampled bool [n], c16 int64 [n, 3], texels int64 [n, 4, 3]: the four texels' bytes, zeros where not sampled)"""
    seen, c16, _ = po.sample_image(X, image, depth, intr, R, t, **locate_opts(kw))
    H, W = image.shape[:2]
    with np.errstate(all="ignore"):
        u, v, _, _ = co.project(intr, R, t, X)
    us, vs = np.where(seen, u, 0.0), np.where(seen, v, 0.0)
    x, y = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
    x1, y1 = np.minimum(x + 1, W - 1), np.minimum(y + 1, H - 1)
    img = image.astype(np.int64)
    tex = np.stack([img[y, x], img[y, x1], img[y1, x], img[y1, x1]], 1)
    return seen, c16, np.where(seen[:, None, None], tex, 0)


def image_sums(X, image, depth, intr, R, t, ref16, valid, gains, **kw):
    """the 20 sums of one image as Python integers; gains int64 [3, 2]"""
    o = dict(DEFAULTS, **kw)
    seen, c16, tex = taps(X, image, depth, intr, R, t, **kw)
    seen = seen & (np.asarray(valid) != 0)
    ref = np.asarray(ref16).astype(np.int64)
    out = []
    refused = 0
    for k in range(3):
        unsat = seen & (tex[:, :, k].min(1) >= o["sat_lo"]) & (tex[:, :, k].max(1) <= o["sat_hi"])
        c = c16[:, k]
        d = apply(gains[k][0], gains[k][1], c) - ref[:, k]
        used = unsat & (np.abs(d) <= 256 * o["gate"]) if o["gate"] > 0 else unsat
        refused += int((unsat & ~used).sum())
        cu, ru, du = c[used], ref[used, k], d[used]
        out += [int(used.sum()), int(cu.sum()), int(ru.sum()), int((cu * cu).sum()), int((cu * ru).sum()), int((du * du).sum())]
    return out + [int(seen.sum()), refused]


def sums(points, images, depth, intr, Rcw, tcw, ref16, valid, gains=None, which=None, **kw):
    """uint64 [m, 20] of the images `which` (default: all), gains int64 [M, 3, 2] indexed by image (None: identity)"""
    X = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    g = identity(len(images)) if gains is None else np.asarray(gains, np.int64)
    rows = [image_sums(X, images[j], None if depth is None else depth[j], intr, R[j], t[j], ref16, valid, g[j].tolist(), **kw)
            for j in (range(len(images)) if which is None else which)]
    return np.array(rows, np.uint64).reshape(-1, N_SUMS)


def fuse(points, images, depth, intr, Rcw, tcw, gains, **kw):
    """the fusion's sums with gains: (n_views int32 [n], S1 uint32 [n, 3], S2 int64 [n, 3])"""
    X = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    n = len(X)
    nv, S1, S2 = np.zeros(n, np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    for j in range(len(images)):
        seen, c16, _ = po.sample_image(X, images[j], None if depth is None else depth[j], intr, R[j], t[j], **locate_opts(kw))
        c = np.where(seen[:, None], apply(gains[j][:, 0][None], gains[j][:, 1][None], c16), 0)
        nv += seen
        S1 += c
        S2 += c * c
    return nv.astype(np.int32), S1.astype(np.uint32), S2


def reference(nv, S1, min_views=2):
    """(ref16 uint16 [n, 3], valid uint8 [n]): (2 S1 + n) // (2 n), invalid below min_views"""
    n = np.asarray(nv, np.int64)
    s = np.asarray(S1).astype(np.int64)
    valid = n >= max(int(min_views), 1)
    nn = np.where(valid, n, 1)[:, None]
    return np.where(valid[:, None], (2 * s + nn) // (2 * nn), 0).astype(np.uint16), valid.astype(np.uint8)


def limits(o):
    return (int(math.floor(o["min_gain"] * 65536.0 + 0.5)), int(math.floor(o["max_gain"] * 65536.0 + 0.5)),
            int(math.floor(o["max_offset"] * 16777216.0 + 0.5)))


def solve_channel(s, o):
    """(state, A, B) of one channel's six sums, Python integers"""
    n, sc, sr, scc, scr = (int(v) for v in s[:5])
    a_lo, a_hi, b_max = limits(o)
    if n < o["min_samples"]:
        return TOO_FEW_SAMPLES, ONE, 0
    state, affine = OK, o["model"] == AFFINE
    D = n * scc - sc * sc
    if affine and D <= n * n * (o["min_spread"] * 256) ** 2:
        state, affine = FALLBACK_GAIN, False
    if affine:
        A = ((n * scr - sc * sr) * ONE + D // 2) // D
    elif scc == 0:
        return OUT_OF_BOUNDS, ONE, 0
    else:
        A = (scr * ONE + scc // 2) // scc
    if A < a_lo or A > a_hi:
        return OUT_OF_BOUNDS, ONE, 0
    B = ((sr * ONE - A * sc) * 2 + n) // (2 * n) if affine else 0
    if abs(B) > b_max:
        return OUT_OF_BOUNDS, ONE, 0
    return state, A, B


def solve(sums_, **kw):
    """(gains int64 [m, 3, 2], status int32 [m]) of sums [m, 20], on Python integers"""
    o = dict(DEFAULTS, **kw)
    rows = [[int(v) for v in r] for r in np.asarray(sums_).reshape(-1, N_SUMS).tolist()]
    m = len(rows)
    gains, status = [[[ONE, 0] for _ in range(3)] for _ in range(m)], [OK] * m
    for j, r in enumerate(rows):
        per = [solve_channel(r[6 * k:6 * k + 6], o) for k in range(3)]
        status[j] = max(p[0] for p in per)
        if status[j] <= FALLBACK_GAIN:
            gains[j] = [[p[1], p[2]] for p in per]
    ok = [j for j in range(m) if status[j] <= FALLBACK_GAIN]
    for k in range(3):
        if not ok:
            break
        sumA = sum(gains[j][k][0] for j in ok)
        S = (len(ok) * (1 << 32) + sumA // 2) // sumA
        for j in ok:
            gains[j][k] = [(gains[j][k][0] * S + 32768) // ONE, (gains[j][k][1] * S + 32768) // ONE]
        T = (2 * sum(gains[j][k][1] for j in ok) + len(ok)) // (2 * len(ok))
        for j in ok:
            gains[j][k][1] -= T
    for j in ok:
        if any(not (A_MIN <= A <= A_MAX and abs(B) <= B_MAX) for A, B in gains[j]):
            status[j], gains[j] = OUT_OF_BOUNDS, [[ONE, 0] for _ in range(3)]
    return np.array(gains, np.int64).reshape(m, 3, 2), np.array(status, np.int32)


def rmse(sums_):
    s = np.asarray(sums_, np.uint64).reshape(-1, N_SUMS)
    n = s[:, 0:18:6].astype(np.float64).sum(1)
    e = s[:, 5:18:6].astype(np.float64).sum(1)
    return np.where(n > 0, np.sqrt(e / np.maximum(n, 1.0)) / 256.0, 0.0)


def spread(nv, S1, S2, min_views=2):
    _, sigma = po.finish(nv, S1, S2, min_views=min_views)
    return po.summary(nv, sigma, min_views=min_views)["mean_sigma"]


def estimate(points, images, depth, intr, Rcw, tcw, rounds=3, min_views=2, **kw):
    """the alternation: dict(gains, status, mean_sigma [rounds + 1], rounds: per round dict(mean_sigma, rmse, max_gain_change,
    status), sums: the last round's)"""
    M = len(images)
    gains, status = identity(M), np.zeros(M, np.int32)
    out = dict(mean_sigma=[], rounds=[])
    s = np.zeros((M, N_SUMS), np.uint64)
    mv = max(int(min_views), 2)
    for _ in range(max(int(rounds), 1)):
        nv, S1, S2 = fuse(points, images, depth, intr, Rcw, tcw, gains, **kw)
        out["mean_sigma"].append(spread(nv, S1, S2, mv))
        ref16, valid = reference(nv, S1, min_views)
        s = sums(points, images, depth, intr, Rcw, tcw, ref16, valid, gains, **kw)
        new, status = solve(s, **kw)
        out["rounds"].append(dict(mean_sigma=out["mean_sigma"][-1], rmse=rmse(s), status=status.copy(),
                                  max_gain_change=float(np.abs(new[:, :, 0] - gains[:, :, 0]).max(initial=0)) / ONE))
        gains = new
    out["mean_sigma"].append(spread(*fuse(points, images, depth, intr, Rcw, tcw, gains, **kw), mv))
    out.update(gains=gains, status=status, sums=s)
    return out


# ---- the rule as plain loops (tiny cases only), on Python integers and the scalar functions of the matcher's oracles
def loops_apply(A, B, c):
    return min(max((A * c + B + 32768) // ONE, 0), C_MAX)


def loops_sums(points, images, depth, intr, Rcw, tcw, ref16, valid, gains=None, **kw):
    """[[20 Python integers] per image]"""
    import match_depth_oracle as mdo
    o = dict(DEFAULTS, **kw)
    M, H, W = images.shape[:3]
    R, t = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    out = []
    with np.errstate(all="ignore"):
        for j in range(M):
            s = [0] * N_SUMS
            g = [[ONE, 0]] * 3 if gains is None else [[int(a), int(b)] for a, b in np.asarray(gains)[j].tolist()]
            for i, p in enumerate(np.asarray(points, np.float32).reshape(-1, 3)):
                X = [float(p[0]), float(p[1]), float(p[2])]
                if not valid[i] or not all(math.isfinite(c) for c in X):
                    continue
                uv = mdo.project(intr, R[j], t[j], np.array(X))
                if uv is None or not (0.0 <= uv[0] < W - 1 and 0.0 <= uv[1] < H - 1):
                    continue
                Z = float(R[j][2, 0]) * X[0] + float(R[j][2, 1]) * X[1] + float(R[j][2, 2]) * X[2] + float(t[j][2])
                if depth is not None:
                    d = mdo.fetch_depth_bilinear(depth[j], np.float32(uv[0]), np.float32(uv[1]))
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
                s[18] += 1
                for k in range(3):
                    tex = [int(images[j, y, x, k]), int(images[j, y, x + 1, k]), int(images[j, y + 1, x, k]), int(images[j, y + 1, x + 1, k])]
                    if min(tex) < o["sat_lo"] or max(tex) > o["sat_hi"]:
                        continue
                    c = ((256 - a) * (256 - b) * tex[0] + a * (256 - b) * tex[1] + (256 - a) * b * tex[2] + a * b * tex[3] + 128) >> 8
                    r = int(ref16[i][k])
                    e = loops_apply(g[k][0], g[k][1], c) - r
                    if o["gate"] > 0 and abs(e) > 256 * o["gate"]:
                        s[19] += 1
                        continue
                    q = 6 * k
                    s[q] += 1; s[q + 1] += c; s[q + 2] += r; s[q + 3] += c * c; s[q + 4] += c * r; s[q + 5] += e * e
            out.append(s)
    return out
