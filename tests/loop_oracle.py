"""CPU restatement of the loop-closure candidate rule (lvba_loop_candidates, csrc/loop_device.h) and of the acceptance rule of
pipeline.find_loop_closures.  TEST INFRASTRUCTURE ONLY.

    S = submap_size; submap w holds frames F_w = [w S, min((w + 1) S, n)); a query j is a multiple of query_stride
    d2(j, f) = ((dx dx + dy dy) + dz dz)                    fp64, this operation order
    (j, w) eligible iff |j - f| >= min_gap for every f in F_w, and min_f d2(j, f) <= radius radius
    ref = the f of the smallest d2 (the lowest f on a tie); per query the max_per_frame smallest (d2, w); output by (query, submap)
"""
from __future__ import annotations

import numpy as np


def d2_matrix(poses):
    p = np.asarray(poses, np.float64).reshape(-1, 12)[:, 9:]
    dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def pairs(poses, submap_size, min_gap, radius, query_stride=1):
    """Every (query, submap) pair with its verdicts: list of dict(query, submap, ref, d2, gap_ok, radius_ok)."""
    n = len(np.asarray(poses).reshape(-1, 12))
    D = d2_matrix(poses)
    r2 = float(radius) * float(radius)
    out = []
    for j in range(0, n, query_stride):
        for w in range((n + submap_size - 1) // submap_size):
            f0, f1 = w * submap_size, min((w + 1) * submap_size, n)
            gap_ok = all(abs(j - f) >= min_gap for f in range(f0, f1))
            ref = f0 + int(np.argmin(D[j, f0:f1]))                        # argmin: the first of equal minima
            out.append(dict(query=j, submap=w, ref=ref, d2=float(D[j, ref]), gap_ok=gap_ok, radius_ok=bool(D[j, ref] <= r2)))
    return out


def candidates(poses, submap_size=10, min_gap=50, max_per_frame=2, query_stride=1, radius=5.0):
    """[(query, submap, ref, distance)] in output order."""
    el = [p for p in pairs(poses, submap_size, min_gap, radius, query_stride) if p["gap_ok"] and p["radius_ok"]]
    out = []
    for j in sorted({p["query"] for p in el}):
        mine = sorted((p for p in el if p["query"] == j), key=lambda p: (p["d2"], p["submap"]))[:max_per_frame]
        out += [(p["query"], p["submap"], p["ref"], float(np.sqrt(p["d2"]))) for p in sorted(mine, key=lambda p: p["submap"])]
    return out


def decision_margin(poses, submap_size, min_gap, radius, query_stride=1):
    """Smallest relative distance of any d2 that takes part in a decision to what it is compared with: radius^2, and the d2 of
    a competing frame of the same submap or of a competing eligible submap of the same query."""
    el = [p for p in pairs(poses, submap_size, min_gap, radius, query_stride) if p["gap_ok"]]
    D = d2_matrix(poses)
    n = len(D)
    r2 = float(radius) ** 2
    m = np.inf
    for p in el:
        m = min(m, abs(p["d2"] - r2) / r2)
        f0, f1 = p["submap"] * submap_size, min((p["submap"] + 1) * submap_size, n)
        for f in range(f0, f1):
            if f != p["ref"]:
                m = min(m, abs(D[p["query"], f] - p["d2"]) / max(p["d2"], 1e-300))
        for q in el:
            if q["query"] == p["query"] and q["submap"] != p["submap"] and p["radius_ok"] and q["radius_ok"]:
                m = min(m, abs(q["d2"] - p["d2"]) / max(p["d2"], 1e-300))
    return float(m)


def correction(T0, T):
    """(rotation angle of R0^T R, |t - t0|)."""
    T0, T = np.asarray(T0, np.float64).reshape(12), np.asarray(T, np.float64).reshape(12)
    dR = T0[:9].reshape(3, 3).T @ T[:9].reshape(3, 3)
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(T[9:] - T0[9:]))


def accept(status, inliers, points, rmse, rot, trans, min_inlier_frac=0.3, max_rmse=None, max_rot=None, max_trans=None):
    """(accepted, reason): converged, enough inliers, rmse and correction within the bounds that are given; the first clause
    that fails names the reason."""
    if status != 0:
        return False, "status"
    if inliers < min_inlier_frac * points:
        return False, "inliers"
    if max_rmse is not None and rmse > max_rmse:
        return False, "rmse"
    if (max_rot is not None and rot > max_rot) or (max_trans is not None and trans > max_trans):
        return False, "correction"
    return True, None
