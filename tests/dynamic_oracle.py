"""numpy restatement of the dynamic-point rule (include/lvba_hip.h, "Moving objects in the LiDAR map"; csrc/dynamic_device.h)
with plain loops over frames: range images, dilation, votes, labels and the selection.  Everything is fp64 on fp32 points
promoted once, every expression written as the header writes it.  It also returns the MARGINS: the relative distance of every
decision from its boundary -- of every own-frame point and every query projection from the range, elevation, row and column
boundaries, of both tolerance comparisons and of the ratio test.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

PI = 3.14159265358979323846
DEFAULTS = dict(n_rows=240, n_cols=720, el_min=-PI / 3.0, el_max=PI / 3.0, min_range=0.5, max_range=80.0, abs_tol=0.2, rel_tol=0.02,
                halo=1, window=20, min_free=3, free_ratio=0.5)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    return o


def _grid_margin(u, n):
    """relative distance of u from the nearest boundary between two of the n cells (the integers 1 .. n - 1; floor(u) is
    clamped to n - 1, and u < 0 does not occur: the two ends are no boundaries)"""
    k = np.round(u)
    return np.where((k >= 1) & (k <= n - 1), np.abs(u - k) / np.maximum(np.abs(u), 1.0), np.inf)


def cells(xyz, **kw):
    """xyz [n, 3] float64 body-frame points: cell (row * n_cols + col, -1 without one), r, margin per point"""
    o = options(**kw)
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        s = x * x + y * y
        rho, r = np.sqrt(s), np.sqrt(s + z * z)
        in_range = np.isfinite(r) & (r >= o["min_range"]) & (r < o["max_range"])
        off_axis = rho > 0.0
        u = (np.arctan2(y, x) + PI) * float(o["n_cols"]) / (2.0 * PI)
        col = np.minimum(np.floor(u), o["n_cols"] - 1)
        e = np.arctan2(z, rho)
        in_el = (e >= o["el_min"]) & (e < o["el_max"])
        v = (e - o["el_min"]) * float(o["n_rows"]) / (o["el_max"] - o["el_min"])
        row = np.minimum(np.floor(v), o["n_rows"] - 1)
        m_rng = np.minimum(np.abs(r - o["min_range"]) / max(o["min_range"], 1e-300), np.abs(r - o["max_range"]) / o["max_range"])
        m_el = np.minimum(np.abs(e - o["el_min"]) / max(abs(o["el_min"]), 1.0), np.abs(e - o["el_max"]) / max(abs(o["el_max"]), 1.0))
        m_cell = np.minimum(_grid_margin(u, o["n_cols"]), _grid_margin(v, o["n_rows"]))
    keep = in_range & off_axis & in_el
    # a non-finite range and rho == 0 are exact on every implementation; then the first failing clause decides alone
    margin = np.where(~np.isfinite(r), np.inf,
                      np.where(~in_range, m_rng,
                               np.where(~off_axis, np.inf,
                                        np.where(~in_el, np.minimum(m_rng, m_el), np.minimum(np.minimum(m_rng, m_el), m_cell)))))
    cell = np.where(keep, np.where(keep, row, 0) * o["n_cols"] + np.where(keep, col, 0), -1).astype(np.int64)
    return dict(cell=cell, r=r, margin=margin)


def range_image(cloud, **kw):
    """I [n_rows, n_cols] float32 of one frame's cloud [n, >=3] float32, +inf where no point falls; and cells() of its points"""
    o = options(**kw)
    c = cells(np.asarray(cloud, np.float32)[:, :3].astype(np.float64), **o)
    img = np.full(o["n_rows"] * o["n_cols"], np.inf, np.float32)
    for k in np.flatnonzero(c["cell"] >= 0):
        img[c["cell"][k]] = min(img[c["cell"][k]], np.float32(c["r"][k]))
    return img.reshape(o["n_rows"], o["n_cols"]), c


def dilate(img, halo):
    """M: the minimum over rows row - halo .. row + halo (clipped) and columns col - halo .. col + halo (modulo n_cols)"""
    n_rows = img.shape[0]
    out = img.copy()
    for dr in range(-halo, halo + 1):
        for dc in range(-halo, halo + 1):
            shifted = np.roll(img, -dc, axis=1)                       # shifted[:, c] = img[:, (c + dc) % n_cols]
            lo, hi = max(0, -dr), min(n_rows, n_rows - dr)             # rows whose neighbour row + dr exists
            out[lo:hi] = np.minimum(out[lo:hi], shifted[lo + dr:hi + dr])
    return out


def world_points(cloud, T):
    p = np.asarray(cloud, np.float32)[:, :3].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([T[0] * x + T[1] * y + T[2] * z + T[9], T[3] * x + T[4] * y + T[5] * z + T[10],
                         T[6] * x + T[7] * y + T[8] * z + T[11]], 1)


def to_body(w, T):
    with np.errstate(all="ignore"):
        d0, d1, d2 = w[:, 0] - T[9], w[:, 1] - T[10], w[:, 2] - T[11]
        return np.stack([T[0] * d0 + T[3] * d1 + T[6] * d2, T[1] * d0 + T[4] * d1 + T[7] * d2, T[2] * d0 + T[5] * d1 + T[8] * d2], 1)


def _rel(a, b):
    with np.errstate(all="ignore"):
        return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def labels(clouds, poses, frame_begin=0, n_frames=None, **kw):
    """The labels of frames [frame_begin, frame_begin + n_frames) of clouds at poses [n_frames, 12] (relative to frame_begin):
    label uint8, n_free, n_support int32 [P] in cloud order, the summary counts, the images I and M per frame, the cell of every
    own-frame point, and margin = the smallest margin of any decision taken."""
    o = options(**kw)
    nf = len(clouds) - frame_begin if n_frames is None else n_frames
    use = [np.asarray(c, np.float32)[:, :3] for c in clouds[frame_begin:frame_begin + nf]]
    T = np.asarray(poses, np.float64).reshape(nf, 12)
    margin = np.inf
    I, M, own = [], [], []
    for c in use:
        img, info = range_image(c, **o)
        I.append(img); M.append(dilate(img, o["halo"])); own.append(info["cell"])
        if len(c):
            margin = min(margin, float(info["margin"].min()))
    free, support = [], []
    for f, c in enumerate(use):
        w = world_points(c, T[f])
        n_free, n_support = np.zeros(len(c), np.int32), np.zeros(len(c), np.int32)
        g0 = 0 if o["window"] <= 0 else max(0, f - o["window"])
        g1 = nf if o["window"] <= 0 else min(nf, f + o["window"] + 1)
        for g in range(g0, g1):
            if g == f or not len(c):
                continue
            q = cells(to_body(w, T[g]), **o)
            margin = min(margin, float(q["margin"].min()))
            has = q["cell"] >= 0
            m = np.where(has, M[g].reshape(-1)[np.where(has, q["cell"], 0)], np.inf).astype(np.float64)
            seen = has & np.isfinite(m)
            with np.errstate(all="ignore"):
                tol = o["abs_tol"] + o["rel_tol"] * q["r"]
                hi, lo = q["r"] + tol, q["r"] - tol
                is_free = seen & (m > hi)
                is_support = seen & ~is_free & (m >= lo)
            if seen.any():
                margin = min(margin, float(np.minimum(_rel(m, hi), _rel(m, lo))[seen].min()))
            n_free += is_free; n_support += is_support
        free.append(n_free); support.append(n_support)
    n_free = np.concatenate(free) if free else np.zeros(0, np.int32)
    n_support = np.concatenate(support) if support else np.zeros(0, np.int32)
    total = o["free_ratio"] * (n_free + n_support).astype(np.float64)
    label = ((n_free >= o["min_free"]) & (n_free.astype(np.float64) >= total)).astype(np.uint8)
    decisive = n_free >= o["min_free"]                                 # below min_free the integer comparison decides alone
    if decisive.any():
        margin = min(margin, float((np.abs(n_free - total) / np.maximum(total, 1.0))[decisive].min()))
    return dict(label=label, n_free=n_free, n_support=n_support, n_points=len(label), n_judged=int(((n_free + n_support) > 0).sum()),
                n_dynamic=int(label.sum()), I=I, M=M, own_cell=own, margin=margin)


def select(clouds, keep):
    """Every frame's points with keep != 0 (keep: one entry per point of all clouds, in cloud order), in scan order -- plain
    loops."""
    out, at = [], 0
    for c in clouds:
        c = np.asarray(c, np.float32)[:, :3]
        rows = [c[k] for k in range(len(c)) if keep[at + k]]
        out.append(np.array(rows, np.float32).reshape(-1, 3))
        at += len(c)
    return out
