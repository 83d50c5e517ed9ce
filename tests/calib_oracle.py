"""numpy restatement of the extrinsic refinement's rule (include/lvba_hip.h "LiDAR-camera extrinsic refinement", DESIGN.md §10o;
csrc/calib_device.h).  The per-record terms are written in the header's order, expression for expression: with the trivial and the
Huber loss they are the header's bits (+, -, *, / and sqrt only).  The sums over the records are taken one after another, in index
order or in reversed order -- the device takes a tree, and what the order alone changes is what the two orders here differ by."""
import numpy as np

NS, G0, COST, CNT, SSQ, SW = 31, 21, 27, 28, 29, 30
MIN_DEPTH = 1e-12
EIG_FLOOR = 1e-20
CONVERGED, MAX_ITERATIONS, TOO_FEW_RECORDS, DEGENERATE, RUNNING = 0, 1, 2, 3, -1
TRIVIAL, HUBER = 0, 1
DEFAULTS = dict(max_iterations=20, loss_kind=HUBER, min_records=100, loss_scale_px=2.0, max_error_px=0.0, min_eig_ratio=1e-6,
                eps_rot=1e-10, eps_trans=1e-10)


def options(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def undistort(intr, uv):
    """trk_undistort of tracks_device.h over fp32 pixels [n, 2], operation for operation: fp64 [n, 2], NaN where it fails"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (float(v) for v in intr)
    uv = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64)
    u, v = uv[:, 0], uv[:, 1]
    with np.errstate(all="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & (abs(fx) >= 1e-12) & (abs(fy) >= 1e-12)
        xd, yd = (u - cx) / fx, (v - cy) / fy
        xu, yu = xd.copy(), yd.copy()
        for _ in range(8):
            r2 = xu * xu + yu * yu
            r4 = r2 * r2
            radial = 1.0 + k1 * r2 + k2 * r4
            ok &= ~((np.abs(radial) < 1e-12) | ~np.isfinite(radial))
            xt = 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu)
            yt = p1 * (r2 + 2.0 * yu * yu) + 2.0 * p2 * xu * yu
            xu, yu = (xd - xt) / radial, (yd - yt) / radial
            ok &= np.isfinite(xu) & np.isfinite(yu)
    out = np.stack([xu, yu], 1)
    out[~ok] = np.nan
    return out


def targets(intr, uv, Xb):
    """cal_target: the undistorted target pixel of every record, NaN where the record is unusable"""
    xy = undistort(intr, uv)
    xy[~np.isfinite(np.asarray(Xb, np.float64).reshape(-1, 3)).all(axis=1)] = np.nan
    return xy


def pair_transforms(poses, img_a, img_b):
    """cal_pair: A [P, 12] = (R_ab | p_ab) of the body poses [M, 12]"""
    T = np.asarray(poses, np.float64).reshape(-1, 12)
    Ta, Tb = T[np.asarray(img_a, np.int64)], T[np.asarray(img_b, np.int64)]
    A = np.zeros((len(Ta), 12))
    for i in range(3):
        for j in range(3):
            A[:, 3 * i + j] = (Ta[:, i] * Tb[:, j] + Ta[:, 3 + i] * Tb[:, 3 + j]) + Ta[:, 6 + i] * Tb[:, 6 + j]
    d = [Tb[:, 9 + k] - Ta[:, 9 + k] for k in range(3)]
    for i in range(3):
        A[:, 9 + i] = (Ta[:, i] * d[0] + Ta[:, 3 + i] * d[1]) + Ta[:, 6 + i] * d[2]
    return A


def loss(kind, a, s):
    """loss_eval of visual_loss.h, trivial and Huber: (rho, rho') over the array s"""
    if kind == TRIVIAL:
        return s.copy(), np.ones_like(s)
    assert kind == HUBER
    b = a * a
    with np.errstate(all="ignore"):
        r = np.sqrt(s)
        out = s > b
        rho = np.where(out, 2.0 * a * r - b, s)
        w = np.where(out, np.maximum(np.finfo(np.float64).tiny, a / r), 1.0)
    return rho, w


def evaluate(R, t, A, pair, xy, Xb, intr, o):
    """cal_eval over all records: dict(counted bool [n], r [n, 2], J0, J1 [n, 6], rho, w [n]); rows that do not count hold garbage"""
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy = float(intr[0]), float(intr[1])
    Ar = np.asarray(A, np.float64).reshape(-1, 12)[np.asarray(pair, np.int64)]
    A_ = [Ar[:, k] for k in range(12)]
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, np.float64).reshape(-1, 3)
    x, y = xy[:, 0], xy[:, 1]
    X0, X1, X2 = Xb[:, 0], Xb[:, 1], Xb[:, 2]
    with np.errstate(all="ignore"):
        usable = (x == x) & (y == y)
        d0, d1, d2 = X0 - t[0], X1 - t[1], X2 - t[2]
        q0 = (R[0] * d0 + R[3] * d1) + R[6] * d2
        q1 = (R[1] * d0 + R[4] * d1) + R[7] * d2
        q2 = (R[2] * d0 + R[5] * d1) + R[8] * d2
        w0 = ((A_[0] * q0 + A_[1] * q1) + A_[2] * q2) + A_[9]
        w1 = ((A_[3] * q0 + A_[4] * q1) + A_[5] * q2) + A_[10]
        w2 = ((A_[6] * q0 + A_[7] * q1) + A_[8] * q2) + A_[11]
        cx = ((R[0] * w0 + R[1] * w1) + R[2] * w2) + t[0]
        cy = ((R[3] * w0 + R[4] * w1) + R[5] * w2) + t[1]
        cz = ((R[6] * w0 + R[7] * w1) + R[8] * w2) + t[2]
        front = cz > MIN_DEPTH
        iz = 1.0 / cz
        px, py = cx * iz, cy * iz
        r0, r1 = fx * (px - x), fy * (py - y)
        s = r0 * r0 + r1 * r1
        gate = np.ones(len(x), bool) if not o["max_error_px"] > 0.0 else s <= o["max_error_px"] * o["max_error_px"]
        gx, gy = fx * iz, fy * iz
        gz0, gz1 = -(gx * px), -(gy * py)
        a00, a01, a02 = R[0] * gx + R[6] * gz0, R[1] * gx + R[7] * gz0, R[2] * gx + R[8] * gz0
        a10, a11, a12 = R[3] * gy + R[6] * gz1, R[4] * gy + R[7] * gz1, R[5] * gy + R[8] * gz1
        b00 = (A_[0] * a00 + A_[3] * a01) + A_[6] * a02
        b01 = (A_[1] * a00 + A_[4] * a01) + A_[7] * a02
        b02 = (A_[2] * a00 + A_[5] * a01) + A_[8] * a02
        b10 = (A_[0] * a10 + A_[3] * a11) + A_[6] * a12
        b11 = (A_[1] * a10 + A_[4] * a11) + A_[7] * a12
        b12 = (A_[2] * a10 + A_[5] * a11) + A_[8] * a12
        h00 = (R[0] * b00 + R[1] * b01) + R[2] * b02
        h01 = (R[3] * b00 + R[4] * b01) + R[5] * b02
        h02 = (R[6] * b00 + R[7] * b01) + R[8] * b02
        h10 = (R[0] * b10 + R[1] * b11) + R[2] * b12
        h11 = (R[3] * b10 + R[4] * b11) + R[5] * b12
        h12 = (R[6] * b10 + R[7] * b11) + R[8] * b12
        J0 = np.stack([gz0 * cy + (h01 * X2 - h02 * X1), (gx * cz - gz0 * cx) + (h02 * X0 - h00 * X2),
                       -(gx * cy) + (h00 * X1 - h01 * X0), gx - h00, -h01, gz0 - h02], 1)
        J1 = np.stack([(gz1 * cy - gy * cz) + (h11 * X2 - h12 * X1), -(gz1 * cx) + (h12 * X0 - h10 * X2),
                       gy * cx + (h10 * X1 - h11 * X0), -h10, gy - h11, gz1 - h12], 1)
        rho, w = loss(o["loss_kind"], o["loss_scale_px"], s)
    return dict(counted=usable & front & gate, r=np.stack([r0, r1], 1), J0=J0, J1=J1, rho=rho, w=w, s=s)


def terms(e):
    """cal_accumulate: [NS, n], what every record adds to each sum (zero where it does not count)"""
    n = len(e["counted"])
    T = np.zeros((NS, n))
    c = e["counted"]
    J0, J1, r, w = e["J0"][c], e["J1"][c], e["r"][c], e["w"][c]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            T[k, c] = w * (J0[:, a] * J0[:, b] + J1[:, a] * J1[:, b])
            k += 1
        T[G0 + a, c] = w * (J0[:, a] * r[:, 0] + J1[:, a] * r[:, 1])
    T[COST, c] = 0.5 * e["rho"][c]
    T[CNT, c] = 1.0
    T[SSQ, c] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    T[SW, c] = w
    return T


def sums(T, reverse=False, prefixes=None):
    """the NS sums of the terms, one after another from 0.0 in index order (reverse: from the last record to the first).
    prefixes: instead, [len(prefixes), NS] the index-order sums over the first p records for every p in prefixes."""
    if prefixes is not None:
        out = np.zeros((len(prefixes), NS))
        for q in range(NS):
            c = np.concatenate([[0.0], np.cumsum(T[q])])
            out[:, q] = c[np.asarray(prefixes, np.int64)]
        return out
    if T.shape[1] == 0:
        return np.zeros(NS)
    return np.array([np.cumsum(row[::-1] if reverse else row)[-1] for row in T])


def linearize(R, t, A, pair, xy, Xb, intr, o, reverse=False):
    """(s [NS], sum |term| [NS], counted)"""
    e = evaluate(R, t, A, pair, xy, Xb, intr, o)
    T = terms(e)
    return sums(T, reverse), np.abs(T).sum(axis=1), e["counted"]


def expand(s):
    H = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = s[k]
            k += 1
    return H


def jacobi(H):
    """cal_jacobi: (eigenvalues unsorted, V with the vector of eigenvalue k in column k)"""
    A = np.array(H, np.float64)
    n = len(A)
    V = np.eye(n)
    for _ in range(30):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += abs(A[p, q])
        if not off > 0.0:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                app, aqq = A[p, p], A[q, q]
                with np.errstate(over="ignore"):                                  # theta may overflow: then tt is 0, as in C
                    theta = (aqq - app) / (2.0 * apq)
                    tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(tt * tt + 1.0)
                sn = tt * c
                A[p, p] = app - tt * apq
                A[q, q] = aqq + tt * apq
                A[p, q] = A[q, p] = 0.0
                for r in range(n):
                    vp, vq = V[r, p], V[r, q]
                    V[r, p] = c * vp - sn * vq
                    V[r, q] = sn * vp + c * vq
                    if r == p or r == q:
                        continue
                    arp, arq = A[r, p], A[r, q]
                    A[r, p] = A[p, r] = c * arp - sn * arq
                    A[r, q] = A[q, r] = sn * arp + c * arq
    return np.diag(A).copy(), V


def orthonormalise(R):
    """resect_orthonormalise of resect_device.h"""
    R = np.asarray(R, np.float64).reshape(9)
    tr = R[0] + R[4] + R[8]
    if tr >= R[0] and tr >= R[4] and tr >= R[8]:
        w, x, y, z = 1.0 + tr, R[7] - R[5], R[2] - R[6], R[3] - R[1]
    elif R[0] >= R[4] and R[0] >= R[8]:
        w, x, y, z = R[7] - R[5], 1.0 + R[0] - R[4] - R[8], R[1] + R[3], R[2] + R[6]
    elif R[4] >= R[8]:
        w, x, y, z = R[2] - R[6], R[1] + R[3], 1.0 - R[0] + R[4] - R[8], R[5] + R[7]
    else:
        w, x, y, z = R[3] - R[1], R[2] + R[6], R[5] + R[7], 1.0 - R[0] - R[4] + R[8]
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                     2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                     2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)])


def retract(R, t, d):
    """R <- (I + [om]x) R through a unit quaternion, t <- t + om x t + up"""
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    Rn = np.zeros(9)
    for c in range(3):
        Rn[c] = R[c] + (d[1] * R[6 + c] - d[2] * R[3 + c])
        Rn[3 + c] = R[3 + c] + (d[2] * R[c] - d[0] * R[6 + c])
        Rn[6 + c] = R[6 + c] + (d[0] * R[3 + c] - d[1] * R[c])
    tn = np.array([t[0] + (d[1] * t[2] - d[2] * t[1]) + d[3], t[1] + (d[2] * t[0] - d[0] * t[2]) + d[4],
                   t[2] + (d[0] * t[1] - d[1] * t[0]) + d[5]])
    return orthonormalise(Rn), tn


def step(s, o, may_step, R, t, focal2=0.0):
    """cal_step: (state, R, t, dict(n_used, rmse, cost, eig, vec, n_held, held, d))"""
    cnt = s[CNT]
    out = dict(n_used=int(cnt), cost=s[COST], rmse=np.sqrt(s[SSQ] / cnt) if cnt > 0 else 0.0, n_held=0, eig=np.zeros(6),
               vec=np.zeros((6, 6)), held=np.zeros(6, bool), d=np.zeros(6))
    if cnt < o["min_records"]:
        return TOO_FEW_RECORDS, R, t, out
    lam, V = jacobi(expand(s))
    order = []
    for k in range(6):
        j = len(order)
        order.append(k)
        while j > 0 and lam[order[j - 1]] > lam[k]:
            order[j] = order[j - 1]
            j -= 1
        order[j] = k
    out["eig"] = lam[order]
    out["vec"] = V[:, order].T.copy()
    top = out["eig"].max()
    if not top > EIG_FLOOR * cnt * focal2:                                        # focal2 = fx^2 + fy^2
        out["n_held"] = 6
        return DEGENERATE, R, t, out
    bound = o["min_eig_ratio"] * top
    d = np.zeros(6)
    for k in range(6):
        if not out["eig"][k] > bound:
            out["held"][k] = True
            continue
        v = out["vec"][k]
        vg = 0.0
        for a in range(6):
            vg += v[a] * s[G0 + a]
        c = vg / out["eig"][k]
        for a in range(6):
            d[a] -= v[a] * c
    out["n_held"] = int(out["held"].sum())
    out["d"] = d
    if out["n_held"] == 6:
        return DEGENERATE, R, t, out
    dr = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    dt = np.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
    if not (np.isfinite(dr) and np.isfinite(dt)):
        return DEGENERATE, R, t, out
    if dr <= o["eps_rot"] and dt <= o["eps_trans"]:
        return CONVERGED, R, t, out
    if not may_step:
        return MAX_ITERATIONS, R, t, out
    Rn, tn = retract(R, t, d)
    return RUNNING, Rn, tn, out


def solve(poses, img_a, img_b, pair, uv, Xb, intr, R, t, reverse=False, **kw):
    """lvba_calib_extrinsic for one job: dict(R [9], t [3], status, iterations, n_used, rmse_px, cost, n_held, eig, vec, held,
    information [6, 6])"""
    o = options(**kw)
    A = pair_transforms(poses, img_a, img_b)
    xy = targets(intr, uv, Xb)
    R, t = np.asarray(R, np.float64).reshape(9).copy(), np.asarray(t, np.float64).reshape(3).copy()
    for it in range(o["max_iterations"] + 1):
        s, _, _ = linearize(R, t, A, pair, xy, Xb, intr, o, reverse)
        state, R, t, out = step(s, o, it < o["max_iterations"], R, t, float(intr[0]) ** 2 + float(intr[1]) ** 2)
        if state != RUNNING:
            break
    return dict(R=R, t=t, status=state, iterations=it, n_used=out["n_used"], rmse_px=out["rmse"], cost=out["cost"], n_held=out["n_held"],
                eig=out["eig"], vec=out["vec"], held=out["held"], information=expand(s))


def cost(R, t, A, pair, xy, Xb, intr, o):
    """the cost alone, summed by numpy (for finite differences)"""
    e = evaluate(R, t, A, pair, xy, Xb, intr, o)
    return float(0.5 * e["rho"][e["counted"]].sum())


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def perturb(R, t, d):
    """the exact left perturbation Exp(om) R, Exp(om) t + up -- what (I + [om]x) is the first order of"""
    E = rodrigues(d[:3])
    return (E @ np.asarray(R).reshape(3, 3)).reshape(9), E @ np.asarray(t).reshape(3) + np.asarray(d[3:])


def left_difference(R, t, R0, t0):
    """d [6] = (om, up) with (R, t) = (Exp(om) R0, Exp(om) t0 + up)"""
    E = np.asarray(R).reshape(3, 3) @ np.asarray(R0).reshape(3, 3).T
    c = np.clip(0.5 * (np.trace(E) - 1.0), -1.0, 1.0)
    th = np.arccos(c)
    v = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    om = v if th < 1e-9 else v * th / np.sin(th)
    return np.concatenate([om, np.asarray(t).reshape(3) - E @ np.asarray(t0).reshape(3)])
