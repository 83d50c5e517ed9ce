"""numpy restatement of the photometric camera alignment (include/lvba_hip.h, "photometric camera alignment against the coloured
map").

The rule, once more.  A point is sampled in an image exactly as the colour fusion samples it (photo_oracle.sample_image: the same
fate, max_depth, holes, (u, v), x, y, a, b and c16), and only where its validity byte is set.  From the same four texels t00 = (y, x),
t10 = (y, x + 1), t01 = (y + 1, x), t11 = (y + 1, x + 1), per channel, gu = ((256 - b)(t10 - t00) + b (t11 - t01)) / 256 and gv =
((256 - a)(t01 - t00) + a (t11 - t10)) / 256 with integer numerators.  r = (c16 - ref16) / 256.  Xc = R X + t as the projection
writes it; Jpi = the derivative of the projection's (u, v) by Xc, the distortion included; q = gu Jpi[0] + gv Jpi[1]; the row is
(Xc x q, q) in the order (om, up) of the left perturbation R <- (I + [om]x) R, t <- t + om x t + up.  rho = the loss of s = r^2 at
loss_scale.  Sums: H = sum rho' J^T J (upper triangle by row), g = sum rho' J^T r, cost = sum rho / 2, the samples, sum r^2, sum
rho'.  The step and the states are align_image below, statement for statement what csrc/palign_device.h does.

Every per-sample expression is written in the header's order, so the records compare bit for bit; the sums here are numpy's
pairwise ones and `abs_sums` is the sum of the terms' magnitudes, which the device's tree is held against."""
import math

import numpy as np

import covis_oracle as co
import photo_oracle as po

DEFAULTS = dict(occlusion_rel=0.05, occlusion_abs=0.1, max_depth=0.0, loss_scale=10.0, eps_rot=1e-7, eps_trans=1e-6,
                max_rotation_deg=5.0, max_translation=0.5, holes=0, loss_kind=1, min_samples=200, max_iterations=15,
                max_batch_images=0)
PHOTO_KEYS = ("occlusion_rel", "occlusion_abs", "max_depth", "holes")
CONVERGED, MAX_ITERATIONS, TOO_FEW_SAMPLES, DEGENERATE, OUT_OF_BOUNDS = range(5)
NS, G0, COST, CNT, SSQ, SW = 31, 21, 27, 28, 29, 30
LAMBDA0, LAMBDA_MIN, DIAG_FLOOR = 1e-3, 1e-9, 1e-12
DBL_MIN = 2.2250738585072014e-308


def loss(kind, a, s):
    """(rho, rho') of visual_loss.h's loss_eval on the array s: the trivial and the Huber kind"""
    if kind == 0:
        return s.copy(), np.ones_like(s)
    assert kind == 1, "the oracle restates the trivial and the Huber loss"
    b = a * a
    with np.errstate(all="ignore"):
        r = np.sqrt(s)
        out = s > b
        return np.where(out, 2.0 * a * r - b, s), np.where(out, np.maximum(DBL_MIN, a / r), 1.0)


def camera_points(R, t, X):
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return np.stack([R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1] + R[k, 2] * X[:, 2] + t[k] for k in range(3)], 1)


def jpi(intr, Xc):
    """(Ju, Jv) [n, 3]: the derivatives of trk_project_cam's (u, v) by Xc"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(x) for x in intr)
    iz = 1.0 / Xc[:, 2]
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    r4 = r2 * r2
    radial = 1.0 + k1 * r2 + k2 * r4
    dr = k1 + 2.0 * k2 * r2
    a00 = (radial + 2.0 * (x * x) * dr) + (2.0 * p1 * y + 6.0 * p2 * x)
    a01 = 2.0 * (x * y) * dr + (2.0 * p1 * x + 2.0 * p2 * y)
    a11 = (radial + 2.0 * (y * y) * dr) + (6.0 * p1 * y + 2.0 * p2 * x)
    Ju = np.stack([fx * (a00 * iz), fx * (a01 * iz), -(fx * ((a00 * x + a01 * y) * iz))], 1)
    Jv = np.stack([fy * (a01 * iz), fy * (a11 * iz), -(fy * ((a01 * x + a11 * y) * iz))], 1)
    return Ju, Jv


def taps(image, u, v):
    """(a, b int64 [n], t00, t10, t01, t11 int64 [n, 3]) of the pixels (u, v), all inside [0, W - 1) x [0, H - 1)"""
    xf, yf = np.floor(u), np.floor(v)
    a, b = np.floor((u - xf) * 256.0).astype(np.int64), np.floor((v - yf) * 256.0).astype(np.int64)
    x, y = xf.astype(np.int64), yf.astype(np.int64)
    img = image.astype(np.int64)
    return a, b, img[y, x], img[y, x + 1], img[y + 1, x], img[y + 1, x + 1]


def gradient_numerators(a, b, t00, t10, t01, t11):
    nu = (256 - b)[:, None] * (t10 - t00) + b[:, None] * (t11 - t01)
    nv = (256 - a)[:, None] * (t01 - t00) + a[:, None] * (t11 - t10)
    return nu, nv


def records(points, ref16, valid, image, depth, intr, R, t, **kw):
    """One image at one pose: dict(seen bool [n]; and over the m sampled points, in index order: index [m], c16 int64 [m, 3], gu, gv,
    r [m, 3], J [m, 3, 6], rho, w [m, 3] (rho and rho' per channel), u, v [m], margins)"""
    o = dict(DEFAULTS, **kw)
    X = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    seen, c16, margins = po.sample_image(X, image, depth, intr, R, t, **{k: o[k] for k in PHOTO_KEYS})
    seen = seen & (np.asarray(valid).reshape(-1) != 0)
    idx = np.flatnonzero(seen)
    Xs = X[idx]
    u, v, _, ok = co.project(intr, R, t, Xs)
    assert ok.all()
    a, b, t00, t10, t01, t11 = taps(image, u, v)
    nu, nv = gradient_numerators(a, b, t00, t10, t01, t11)
    gu, gv = nu.astype(np.float64) / 256.0, nv.astype(np.float64) / 256.0
    Xc = camera_points(R, t, Xs)
    Ju, Jv = jpi(intr, Xc)
    c = c16[idx]
    r = (c - np.asarray(ref16, np.uint16).reshape(-1, 3)[idx].astype(np.int64)).astype(np.float64) / 256.0
    q = [gu * Ju[:, k, None] + gv * Jv[:, k, None] for k in range(3)]                      # each [m, 3 channels]
    X0, X1, X2 = Xc[:, 0, None], Xc[:, 1, None], Xc[:, 2, None]
    J = np.stack([X1 * q[2] - X2 * q[1], X2 * q[0] - X0 * q[2], X0 * q[1] - X1 * q[0], q[0], q[1], q[2]], 2)
    rho, w = loss(o["loss_kind"], o["loss_scale"], r * r)
    return dict(seen=seen, index=idx, c16=c, gu=gu, gv=gv, r=r, J=J, rho=rho, w=w, u=u, v=v, margins=margins)


def sums_of(rec):
    """(sums [31], abs_sums [31]): the image's sums from its records and the sums of the terms' magnitudes"""
    r, J, rho, w = rec["r"], rec["J"], rec["rho"], rec["w"]
    s, sa = np.zeros(NS), np.zeros(NS)
    k = 0
    for a in range(6):
        wj = w * J[:, :, a]
        for b in range(a, 6):
            term = wj * J[:, :, b]
            s[k], sa[k] = term.sum(), np.abs(term).sum()
            k += 1
        term = wj * r
        s[G0 + a], sa[G0 + a] = term.sum(), np.abs(term).sum()
    s[COST] = sa[COST] = (0.5 * rho).sum()
    s[CNT] = sa[CNT] = float(len(r))
    s[SSQ] = sa[SSQ] = (r * r).sum()
    s[SW] = sa[SW] = w.sum()
    return s, sa


def linearize(points, ref16, valid, image, depth, intr, R, t, **kw):
    rec = records(points, ref16, valid, image, depth, intr, R, t, **kw)
    s, sa = sums_of(rec)
    return dict(sums=s, abs_sums=sa, n_samples=len(rec["index"]), margins=rec["margins"])


def expand(s):
    H = np.zeros((6, 6))
    iu = np.triu_indices(6)
    H[iu] = s[:21]
    H[(iu[1], iu[0])] = s[:21]
    return H


def solve(s, lam):
    """pal_solve: d = -(H + lam diag(max(H_aa, 1e-12)))^-1 g by LDL^T without pivoting, loop for loop; None where it fails"""
    A = expand(s)
    for a in range(6):
        h = A[a, a]
        A[a, a] = h + lam * (h if h > DIAG_FLOOR else DIAG_FLOOR)
    L, D, y, d = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros(6)
    for j in range(6):
        dj = A[j, j]
        for k in range(j):
            dj -= (L[j, k] * L[j, k]) * D[k]
        if not dj > 0.0:
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v -= (L[i, k] * L[j, k]) * D[k]
            L[i, j] = v / dj
    for i in range(6):
        v = -s[G0 + i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * d[k]
        d[i] = v
    return d if np.isfinite(d).all() else None


def orthonormalise(R):
    """resect_orthonormalise on a flat [9]"""
    R = [float(x) for x in R]
    tr = R[0] + R[4] + R[8]
    if tr >= R[0] and tr >= R[4] and tr >= R[8]:
        w, x, y, z = 1.0 + tr, R[7] - R[5], R[2] - R[6], R[3] - R[1]
    elif R[0] >= R[4] and R[0] >= R[8]:
        w, x, y, z = R[7] - R[5], 1.0 + R[0] - R[4] - R[8], R[1] + R[3], R[2] + R[6]
    elif R[4] >= R[8]:
        w, x, y, z = R[2] - R[6], R[1] + R[3], 1.0 - R[0] + R[4] - R[8], R[5] + R[7]
    else:
        w, x, y, z = R[3] - R[1], R[2] + R[6], R[5] + R[7], 1.0 - R[0] - R[4] + R[8]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    if not n > 0.0 or not math.isfinite(n):
        return np.array(R)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                     2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                     2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)])


def retract(R, t, d):
    """pal_retract on flat R [9], t [3]"""
    R, t, d = [float(x) for x in R], [float(x) for x in t], [float(x) for x in d]
    Rn = [0.0] * 9
    for c in range(3):
        Rn[c] = R[c] + (d[1] * R[6 + c] - d[2] * R[3 + c])
        Rn[3 + c] = R[3 + c] + (d[2] * R[c] - d[0] * R[6 + c])
        Rn[6 + c] = R[6 + c] + (d[0] * R[3 + c] - d[1] * R[c])
    tn = [t[0] + (d[1] * t[2] - d[2] * t[1]) + d[3], t[1] + (d[2] * t[0] - d[0] * t[2]) + d[4], t[2] + (d[0] * t[1] - d[1] * t[0]) + d[5]]
    return orthonormalise(Rn), np.array(tn)


def out_of_bounds(R, t, R0, t0, o):
    chord = float(((R - R0) ** 2).sum())
    C, C0 = R.reshape(3, 3).T @ t, R0.reshape(3, 3).T @ t0
    half = 0.5 * math.radians(o["max_rotation_deg"])
    return not chord <= 8.0 * math.sin(half) * math.sin(half) or not float(np.linalg.norm(C - C0)) <= o["max_translation"]


def align_image(points, ref16, valid, image, depth, intr, R0, t0, **kw):
    """pal_step's loop on one image: dict(Rcw [3, 3], tcw [3], status, iterations, accepted, n_samples, rmse_initial, rmse, cost,
    information [6, 6], margins: the smallest margins over every pose that was linearised at, min_gap: the smallest |n_samples -
    min_samples| over those poses)"""
    o = dict(DEFAULTS, **kw)
    R0, t0 = np.asarray(R0, np.float64).reshape(9).copy(), np.asarray(t0, np.float64).reshape(3).copy()
    R, t, Rt, tt = R0.copy(), t0.copy(), R0.copy(), t0.copy()
    lam, passes, accepted, d = LAMBDA0, 0, 0, np.zeros(6)
    cur = first = None
    margins, min_gap = dict(compare=np.inf, texel=np.inf), np.inf
    status = None
    while status is None:
        lin = linearize(points, ref16, valid, image, depth, intr, Rt.reshape(3, 3), tt, **o)
        s = lin["sums"]
        margins = {k: min(margins[k], lin["margins"][k]) for k in margins}
        min_gap = min(min_gap, abs(lin["n_samples"] - o["min_samples"]))
        passes += 1
        n = s[CNT]
        if passes == 1:
            cur = first = s
            if n < o["min_samples"]:
                status = TOO_FEW_SAMPLES
                break
        else:
            if n >= o["min_samples"] and s[COST] / n < cur[COST] / cur[CNT]:
                R, t, cur = Rt, tt, s
                accepted += 1
                lam = max(lam / 3.0, LAMBDA_MIN)
                if out_of_bounds(R, t, R0, t0, o):
                    R, t, cur, status = R0, t0, first, OUT_OF_BOUNDS
                    break
                dr = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                dt = math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
                if dr <= o["eps_rot"] and dt <= o["eps_trans"]:
                    status = CONVERGED
                    break
            else:
                lam = 4.0 * lam
        if passes >= o["max_iterations"]:
            status = MAX_ITERATIONS
            break
        d = solve(cur, lam) if (np.diag(expand(cur)) > 0.0).all() else None
        if d is None:
            R, t, cur, status = R0, t0, first, DEGENERATE
            break
        Rt, tt = retract(R, t, d)
    rmse = lambda q: math.sqrt(q[SSQ] / (3.0 * q[CNT])) if q[CNT] > 0 else 0.0
    return dict(Rcw=R.reshape(3, 3).copy(), tcw=t.copy(), status=status, iterations=passes, accepted=accepted, n_samples=int(cur[CNT]),
                rmse_initial=rmse(first), rmse=rmse(cur), cost=float(cur[COST]), information=expand(cur), margins=margins,
                min_gap=min_gap)


def align(points, ref16, valid, images, depth, intr, Rcw, tcw, **kw):
    """align_image over the images: the per-image dicts stacked, `margins` and `min_gap` reduced over the images"""
    outs = [align_image(points, ref16, valid, images[j], None if depth is None else depth[j], intr, Rcw[j], tcw[j], **kw)
            for j in range(len(images))]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0] if k not in ("margins", "min_gap")}
    res["margins"] = {k: min(o["margins"][k] for o in outs) for k in ("compare", "texel")}
    res["min_gap"] = min(o["min_gap"] for o in outs)
    return res


def pose_errors(Rcw, tcw, R_true, t_true):
    """(rotation error in degrees [m], camera-centre error in metres [m])"""
    Rcw, R_true = np.asarray(Rcw).reshape(-1, 3, 3), np.asarray(R_true).reshape(-1, 3, 3)
    dR = np.einsum("nij,nkj->nik", Rcw, R_true)
    ang = np.degrees(np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)))
    C = -np.einsum("nji,nj->ni", Rcw, np.asarray(tcw).reshape(-1, 3))
    Ct = -np.einsum("nji,nj->ni", R_true, np.asarray(t_true).reshape(-1, 3))
    return ang, np.linalg.norm(C - Ct, axis=1)


def reference_from_sums(n_views, s1, min_views=2):
    """(ref16, valid) from the fusion's sums, on Python-width integers: (2 S1 + n) // (2 n) where n >= min_views"""
    n = np.asarray(n_views, np.int64)
    s = np.asarray(s1).astype(np.int64)
    valid = n >= min_views
    nn = np.where(valid, n, 1)[:, None]
    return np.where(valid[:, None], (2 * s + nn) // (2 * nn), 0).astype(np.uint16), valid.astype(np.uint8)


# ---- plain loops on Python integers and floats (tiny cases only), written independently of the vectorised functions
def loops_gradient(image, u, v, k):
    """(nu, nv, c16) of channel k at pixel (u, v) on Python integers"""
    x, y = int(math.floor(u)), int(math.floor(v))
    a, b = int(math.floor((u - x) * 256.0)), int(math.floor((v - y) * 256.0))
    t00, t10, t01, t11 = (int(image[y, x, k]), int(image[y, x + 1, k]), int(image[y + 1, x, k]), int(image[y + 1, x + 1, k]))
    nu = (256 - b) * (t10 - t00) + b * (t11 - t01)
    nv = (256 - a) * (t01 - t00) + a * (t11 - t10)
    c = (256 - a) * (256 - b) * t00 + a * (256 - b) * t10 + (256 - a) * b * t01 + a * b * t11
    return nu, nv, (c + 128) >> 8
