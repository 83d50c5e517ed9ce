"""numpy restatement of the time offset's rule (include/lvba_hip.h "the camera-LiDAR time offset", DESIGN.md §10o "time offset";
csrc/calib_td_device.h) on top of tests/calib_oracle.py: the body pose at an offset, the pair table's 21-double row, the record's
seventh column, the 39 sums and the 7-parameter step, written in the header's order, expression for expression -- with the trivial
and the Huber loss a record's terms are the header's bits (+, -, *, / and sqrt only)."""
import numpy as np

import calib_oracle as co

N, NS, G0, COST, CNT, SSQ, SW = 7, 39, 28, 35, 36, 37, 38
ROW = 21
OUT_OF_RANGE = 4
DEFAULTS = dict(co.DEFAULTS, eps_td_s=1e-10, max_abs_td_s=0.2)


def options(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def shift_poses(poses, twists, td):
    """cal_td_pose over all images: [M, 12]"""
    T = np.asarray(poses, np.float64).reshape(-1, 12)
    tw = np.asarray(twists, np.float64).reshape(-1, 6)
    td = float(td)
    th0, th1, th2 = td * tw[:, 0], td * tw[:, 1], td * tw[:, 2]
    s = 1.0 + 0.25 * ((th0 * th0 + th1 * th1) + th2 * th2)
    C = [1.0 + (0.5 * -(th1 * th1 + th2 * th2)) / s, (-th2 + 0.5 * (th0 * th1)) / s, (th1 + 0.5 * (th0 * th2)) / s,
         (th2 + 0.5 * (th0 * th1)) / s, 1.0 + (0.5 * -(th0 * th0 + th2 * th2)) / s, (-th0 + 0.5 * (th1 * th2)) / s,
         (-th1 + 0.5 * (th0 * th2)) / s, (th0 + 0.5 * (th1 * th2)) / s, 1.0 + (0.5 * -(th0 * th0 + th1 * th1)) / s]
    out = np.zeros_like(T)
    for i in range(3):
        for j in range(3):
            out[:, 3 * i + j] = (T[:, 3 * i] * C[j] + T[:, 3 * i + 1] * C[3 + j]) + T[:, 3 * i + 2] * C[6 + j]
    for i in range(3):
        out[:, 9 + i] = T[:, 9 + i] + td * tw[:, 3 + i]
    return out


def rates(twists, td):
    """cal_td_rate: om' [M, 3]"""
    tw = np.asarray(twists, np.float64).reshape(-1, 6)
    td = float(td)
    den = 1.0 + 0.25 * ((td * td) * ((tw[:, 0] * tw[:, 0] + tw[:, 1] * tw[:, 1]) + tw[:, 2] * tw[:, 2]))
    return np.stack([tw[:, 0] / den, tw[:, 1] / den, tw[:, 2] / den], 1)


def pair_table(poses, twists, img_a, img_b, td):
    """cal_td_pair: E [P, 21] = (A(td) | om'_a | om'_b | dv)"""
    a, b = np.asarray(img_a, np.int64), np.asarray(img_b, np.int64)
    S = shift_poses(poses, twists, td)
    tw = np.asarray(twists, np.float64).reshape(-1, 6)
    E = np.zeros((len(a), ROW))
    E[:, :12] = co.pair_transforms(S, a, b)
    r = rates(twists, td)
    E[:, 12:15], E[:, 15:18] = r[a], r[b]
    Sa = S[a]
    e = [tw[b, 3 + k] - tw[a, 3 + k] for k in range(3)]
    for i in range(3):
        E[:, 18 + i] = (Sa[:, i] * e[0] + Sa[:, 3 + i] * e[1]) + Sa[:, 6 + i] * e[2]
    return E


def evaluate(R, t, E, pair, xy, Xb, intr, o):
    """cal_td_eval over all records: calib_oracle.evaluate's dict with J0, J1 [n, 7]"""
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    E = np.asarray(E, np.float64).reshape(-1, ROW)
    e = co.evaluate(R, t, E[:, :12], pair, xy, Xb, intr, o)
    fx, fy = float(intr[0]), float(intr[1])
    Er = E[np.asarray(pair, np.int64)]
    A_ = [Er[:, k] for k in range(12)]
    oa, ob, dv = Er[:, 12:15], Er[:, 15:18], Er[:, 18:21]
    Xb = np.asarray(Xb, np.float64).reshape(-1, 3)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        # cal_eval's intermediates again, in its order
        d0, d1, d2 = Xb[:, 0] - t[0], Xb[:, 1] - t[1], Xb[:, 2] - t[2]
        q0 = (R[0] * d0 + R[3] * d1) + R[6] * d2
        q1 = (R[1] * d0 + R[4] * d1) + R[7] * d2
        q2 = (R[2] * d0 + R[5] * d1) + R[8] * d2
        w0 = ((A_[0] * q0 + A_[1] * q1) + A_[2] * q2) + A_[9]
        w1 = ((A_[3] * q0 + A_[4] * q1) + A_[5] * q2) + A_[10]
        w2 = ((A_[6] * q0 + A_[7] * q1) + A_[8] * q2) + A_[11]
        cx = ((R[0] * w0 + R[1] * w1) + R[2] * w2) + t[0]
        cy = ((R[3] * w0 + R[4] * w1) + R[5] * w2) + t[1]
        cz = ((R[6] * w0 + R[7] * w1) + R[8] * w2) + t[2]
        iz = 1.0 / cz
        px, py = cx * iz, cy * iz
        gx, gy = fx * iz, fy * iz
        gz0, gz1 = -(gx * px), -(gy * py)
        a00, a01, a02 = R[0] * gx + R[6] * gz0, R[1] * gx + R[7] * gz0, R[2] * gx + R[8] * gz0
        a10, a11, a12 = R[3] * gy + R[6] * gz1, R[4] * gy + R[7] * gz1, R[5] * gy + R[8] * gz1
        c0 = ob[:, 1] * q2 - ob[:, 2] * q1
        c1 = ob[:, 2] * q0 - ob[:, 0] * q2
        c2 = ob[:, 0] * q1 - ob[:, 1] * q0
        e0 = oa[:, 1] * w2 - oa[:, 2] * w1
        e1 = oa[:, 2] * w0 - oa[:, 0] * w2
        e2 = oa[:, 0] * w1 - oa[:, 1] * w0
        dw0 = (((A_[0] * c0 + A_[1] * c1) + A_[2] * c2) - e0) + dv[:, 0]
        dw1 = (((A_[3] * c0 + A_[4] * c1) + A_[5] * c2) - e1) + dv[:, 1]
        dw2 = (((A_[6] * c0 + A_[7] * c1) + A_[8] * c2) - e2) + dv[:, 2]
        j0 = (a00 * dw0 + a01 * dw1) + a02 * dw2
        j1 = (a10 * dw0 + a11 * dw1) + a12 * dw2
    e["J0"] = np.concatenate([e["J0"], j0[:, None]], 1)
    e["J1"] = np.concatenate([e["J1"], j1[:, None]], 1)
    return e


def terms(e):
    """cal_td_accumulate: [NS, n], what every record adds to each sum (zero where it does not count)"""
    n = len(e["counted"])
    T = np.zeros((NS, n))
    c = e["counted"]
    J0, J1, r, w = e["J0"][c], e["J1"][c], e["r"][c], e["w"][c]
    k = 0
    for a in range(N):
        for b in range(a, N):
            T[k, c] = w * (J0[:, a] * J0[:, b] + J1[:, a] * J1[:, b])
            k += 1
        T[G0 + a, c] = w * (J0[:, a] * r[:, 0] + J1[:, a] * r[:, 1])
    T[COST, c] = 0.5 * e["rho"][c]
    T[CNT, c] = 1.0
    T[SSQ, c] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    T[SW, c] = w
    return T


def sums(T, reverse=False):
    """the NS sums of the terms, one after another from 0.0 in index order (reverse: from the last record to the first)"""
    if T.shape[1] == 0:
        return np.zeros(len(T))
    return np.array([np.cumsum(row[::-1] if reverse else row)[-1] for row in T])


def linearize(R, t, td, poses, twists, img_a, img_b, pair, xy, Xb, intr, o, reverse=False):
    """(s [NS], sum |term| [NS], counted)"""
    E = pair_table(poses, twists, img_a, img_b, td)
    e = evaluate(R, t, E, pair, xy, Xb, intr, o)
    T = terms(e)
    return sums(T, reverse), np.abs(T).sum(axis=1), e["counted"]


def expand(s, n=N):
    H = np.zeros((n, n))
    k = 0
    for a in range(n):
        for b in range(a, n):
            H[a, b] = H[b, a] = s[k]
            k += 1
    return H


def free_step(n, H, g, min_eig_ratio, floor):
    """cal_free_step: (d or None, eig, vec, held bool [n])"""
    lam, V = co.jacobi(H)
    order = []
    for k in range(n):
        j = len(order)
        order.append(k)
        while j > 0 and lam[order[j - 1]] > lam[k]:
            order[j] = order[j - 1]
            j -= 1
        order[j] = k
    eig, vec = lam[order], V[:, order].T.copy()
    top = eig.max()
    if not top > floor:
        return None, eig, vec, np.ones(n, bool)
    bound = min_eig_ratio * top
    d = np.zeros(n)
    held = np.zeros(n, bool)
    for k in range(n):
        if not eig[k] > bound:
            held[k] = True
            continue
        v = vec[k]
        vg = 0.0
        for a in range(n):
            vg += v[a] * g[a]
        c = vg / eig[k]
        for a in range(n):
            d[a] -= v[a] * c
    return (None if held.all() else d), eig, vec, held


def step(s, o, may_step, R, t, td, focal2=0.0):
    """cal_td_step: (state, R, t, td, dict(n_used, rmse, cost, eig, vec, n_held, held, d))"""
    cnt = s[CNT]
    out = dict(n_used=int(cnt), cost=s[COST], rmse=np.sqrt(s[SSQ] / cnt) if cnt > 0 else 0.0, n_held=0, eig=np.zeros(N),
               vec=np.zeros((N, N)), held=np.zeros(N, bool), d=np.zeros(N))
    if cnt < o["min_records"]:
        return co.TOO_FEW_RECORDS, R, t, td, out
    d, out["eig"], out["vec"], out["held"] = free_step(N, expand(s), s[G0:G0 + N], o["min_eig_ratio"], co.EIG_FLOOR * cnt * focal2)
    out["n_held"] = int(out["held"].sum())
    if d is None:
        return co.DEGENERATE, R, t, td, out
    out["d"] = d
    dr = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    dt = np.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
    if not (np.isfinite(dr) and np.isfinite(dt) and np.isfinite(d[6])):
        return co.DEGENERATE, R, t, td, out
    if dr <= o["eps_rot"] and dt <= o["eps_trans"] and abs(d[6]) <= o["eps_td_s"]:
        return co.CONVERGED, R, t, td, out
    if not may_step:
        return co.MAX_ITERATIONS, R, t, td, out
    tn = td + d[6]
    if abs(tn) > o["max_abs_td_s"]:
        return OUT_OF_RANGE, R, t, td, out
    Rn, tt = co.retract(R, t, d)
    return co.RUNNING, Rn, tt, tn, out


def solve(poses, twists, img_a, img_b, pair, uv, Xb, intr, R, t, td=0.0, reverse=False, **kw):
    """lvba_calib_extrinsic_td for one job: dict(R [9], t [3], td, status, iterations, n_used, rmse_px, cost, n_held, eig, vec, held,
    information [7, 7], s)"""
    o = options(**kw)
    xy = co.targets(intr, uv, Xb)
    R0, t0, td0 = np.asarray(R, np.float64).reshape(9).copy(), np.asarray(t, np.float64).reshape(3).copy(), float(td)
    R, t, td = R0, t0, td0
    for it in range(o["max_iterations"] + 1):
        s, _, _ = linearize(R, t, td, poses, twists, img_a, img_b, pair, xy, Xb, intr, o, reverse)
        state, R, t, td, out = step(s, o, it < o["max_iterations"], R, t, td, float(intr[0]) ** 2 + float(intr[1]) ** 2)
        if state != co.RUNNING:
            break
    if state == OUT_OF_RANGE:
        R, t, td = R0, t0, td0
    return dict(R=R, t=t, td=td, status=state, iterations=it, n_used=out["n_used"], rmse_px=out["rmse"], cost=out["cost"],
                n_held=out["n_held"], eig=out["eig"], vec=out["vec"], held=out["held"], information=expand(s), s=s)
