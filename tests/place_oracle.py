"""CPU restatement of the scan-descriptor place recognition (lvba_place_*, csrc/place_device.h; include/lvba_hip.h has the
definitions).  TEST INFRASTRUCTURE ONLY.

    descriptor   D[ring][sector] = max(0, max (float)(z + z_offset)) over the points with min_range <= r < max_range
    ring key     key[ring] = (float)((double)#(D > 0) / Ns)
    columns      U[:, j] = D[:, j] / sqrt(sum_ring D[ring][j]^2), the sum in ring order, fp64; a zero column is empty
    distance     dist(s) = 1 - sim(s) / n(s), sim over the columns where neither side is empty in (j, ring) order; the smallest s
                 of the smallest dist is the shift
    candidates   the K smallest (fp32 key distance, f) among the frames of submaps that pass the gap clause; per submap the
                 smallest (dist, f); dist <= max_distance; per query the max_per_frame smallest (dist, w); output by (query, w)

Sums whose order matters run in explicit loops over their terms (vectorised only across independent sums).
"""
from __future__ import annotations

import numpy as np

PI = 3.14159265358979323846
DEFAULTS = dict(n_rings=20, n_sectors=60, min_range=0.5, max_range=80.0, z_offset=2.0, submap_size=10, min_gap=50, n_key_candidates=10,
                max_per_frame=2, query_stride=1, max_distance=0.4)


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        if k not in o:
            raise TypeError(k)
    o.update(kw)
    return o


def bins(cloud, **kw):
    """Per point: keep (bool), ring, sector, h (fp32), and the relative distance of the point to the nearest ring, sector and
    range boundary (inf for the points that the range drops by more than that)."""
    o = options(**kw)
    nr, ns = o["n_rings"], o["n_sectors"]
    p = np.asarray(cloud, np.float32)[:, :3].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = np.sqrt(x * x + y * y)
    with np.errstate(invalid="ignore"):
        keep = (r >= o["min_range"]) & (r < o["max_range"])
        h = (z + o["z_offset"]).astype(np.float32)
        keep &= (h > 0) & (h < np.inf)
        fr = r * float(nr) / o["max_range"]
        fs = (np.arctan2(y, x) + PI) * float(ns) / (2.0 * PI)
    ring = np.minimum(np.floor(np.where(keep, fr, 0.0)).astype(np.int64), nr - 1)
    sector = np.minimum(np.floor(np.where(keep, fs, 0.0)).astype(np.int64), ns - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m_ring = np.abs(fr - np.round(fr)) / np.maximum(np.abs(fr), 1.0)
        m_sec = np.abs(fs - np.round(fs)) / np.maximum(np.abs(fs), 1.0)
        m_rng = np.minimum(np.abs(r - o["min_range"]) / max(o["min_range"], 1e-300), np.abs(r - o["max_range"]) / o["max_range"])
    margin = np.where(keep, np.minimum(np.minimum(m_ring, m_sec), m_rng), m_rng)
    return dict(keep=keep, ring=ring, sector=sector, h=h, margin=margin)


def descriptor(cloud, **kw):
    """(D [Nr, Ns] float32, key [Nr] float32) of one cloud [n, >= 3]."""
    o = options(**kw)
    b = bins(cloud, **kw)
    D = np.zeros((o["n_rings"], o["n_sectors"]), np.float32)
    k = b["keep"]
    np.maximum.at(D, (b["ring"][k], b["sector"][k]), b["h"][k])
    return D, ring_key(D)


def ring_key(D):
    D = np.asarray(D, np.float32)
    return ((D > 0).sum(-1).astype(np.float64) / float(D.shape[-1])).astype(np.float32)


def columns(D):
    """(U [Nr, Ns] float64, full [Ns] bool) of a descriptor."""
    D = np.asarray(D, np.float32).astype(np.float64)
    s = np.zeros(D.shape[1])
    for r in range(D.shape[0]):
        s = s + D[r] * D[r]
    norm = np.sqrt(s)
    full = norm > 0
    U = np.where(full, D / np.where(full, norm, 1.0), 0.0)
    return U, full


def shift_distances(Dq, Dc):
    """dist(s) for s = 0 .. Ns - 1, for a batch of pairs: Dq, Dc [P, Nr, Ns] -> [P, Ns]."""
    Dq, Dc = np.asarray(Dq, np.float32), np.asarray(Dc, np.float32)
    if Dq.ndim == 2:
        return shift_distances(Dq[None], Dc[None])[0]
    P, nr, ns = Dq.shape
    Uq, Fq = zip(*(columns(d) for d in Dq))
    Uc, Fc = zip(*(columns(d) for d in Dc))
    Uq, Fq, Uc, Fc = np.stack(Uq), np.stack(Fq), np.stack(Uc), np.stack(Fc)
    s = np.arange(ns)
    sim, cnt = np.zeros((P, ns)), np.zeros((P, ns), np.int64)
    for j in range(ns):
        jq = (j - s) % ns                                                      # roll(U_q, s)[:, j] = U_q[:, (j - s) mod Ns]
        both = Fq[:, jq] & Fc[:, j][:, None]
        cnt += both
        for r in range(nr):
            sim = np.where(both, sim + Uq[:, r, jq] * Uc[:, r, j][:, None], sim)
    return np.where(cnt > 0, 1.0 - sim / np.maximum(cnt, 1), 1.0)


def yaw_of(shift, ns):
    y = 2.0 * PI * float(shift) / float(ns)
    return y - 2.0 * PI if y > PI else y


def key_d2(keys, j):
    """fp32 key distances of query j to every frame, the sum in ring order."""
    keys = np.asarray(keys, np.float32)
    acc = np.zeros(len(keys), np.float32)
    for r in range(keys.shape[1]):
        d = keys[j, r] - keys[:, r]
        acc = acc + d * d
    return acc


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def candidates(desc, with_margin=False, **kw):
    """[(query, submap, ref, shift, distance, yaw)] in output order over descriptors desc [n, Nr, Ns].  with_margin: also the
    smallest relative distance between two UNEQUAL values that a decision compares (the K-th and the (K + 1)-th key distance,
    the best and the second-best dist(s), the refs of a submap, the max_distance gate, the per-query cut)."""
    o = options(**kw)
    desc = np.asarray(desc, np.float32)
    n = len(desc)
    S, K, ns = o["submap_size"], o["n_key_candidates"], o["n_sectors"]
    keys = np.stack([ring_key(d) for d in desc]) if n else np.zeros((0, o["n_rings"]), np.float32)
    picks = {}
    margin = [np.inf]

    def note(a, b):
        if a != b:
            margin[0] = min(margin[0], _rel(float(a), float(b)))

    for j in range(0, n, o["query_stride"]):
        ok = [f for f in range(n) if all(abs(j - g) >= o["min_gap"] for g in range(f // S * S, min((f // S + 1) * S, n)))]
        if not ok:
            continue
        d2 = key_d2(keys, j)
        order = sorted(ok, key=lambda f: (d2[f], f))
        picks[j] = order[:K]
        if len(order) > K:
            note(d2[order[K - 1]], d2[order[K]])
    pairs = [(j, f) for j in picks for f in picks[j]]
    dist = shift_distances(desc[[p[0] for p in pairs]], desc[[p[1] for p in pairs]]) if pairs else np.zeros((0, ns))
    best = {}
    for (j, f), d in zip(pairs, dist):
        s = int(np.argmin(d))                                                 # argmin: the first of equal minima
        best[(j, f)] = (float(d[s]), s)
        for v in d:
            note(d[s], v)
    out = []
    for j in sorted(picks):
        sub = {}
        for f in picks[j]:
            sub.setdefault(f // S, []).append((best[(j, f)][0], f))
        refs = []
        for w, lst in sub.items():
            lst.sort()
            for a in lst[1:]:
                note(lst[0][0], a[0])
            note(lst[0][0], o["max_distance"])
            if lst[0][0] <= o["max_distance"]:
                refs.append((lst[0][0], w, lst[0][1]))
        refs.sort()
        for a in refs[o["max_per_frame"]:]:
            note(refs[o["max_per_frame"] - 1][0], a[0])
        for d, w, f in sorted(refs[:o["max_per_frame"]], key=lambda t: t[1]):
            s = best[(j, f)][1]
            out.append((j, w, f, s, d, yaw_of(s, ns)))
    return (out, margin[0]) if with_margin else out


def rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def start_pose(pose_ref, yaw):
    """T_init = T_ref o (Rz(yaw), 0) as [12]."""
    T = np.asarray(pose_ref, np.float64).reshape(12)
    return np.r_[(T[:9].reshape(3, 3) @ rz(yaw)).reshape(9), T[9:]]
