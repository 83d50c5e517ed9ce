"""Camera resectioning on the GPU: the absolute pose of many images at once from 2-D to 3-D correspondences, by batched P3P RANSAC
(lvba_resect_*; the rule is in include/lvba_hip.h).  Opt-in: nothing imports this module unless resectioning is
asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.ResectOpts)
OK, TOO_FEW_MATCHES, NO_MODEL, TOO_FEW_INLIERS = 0, 1, 2, 3
STATUS_NAMES = ("ok", "too_few_matches", "no_model", "too_few_inliers")


def resect_opts(lib=None, **kw):
    """lvba_resect_opts: the defaults (1024 hypotheses, 2 refinement rounds, 30 inliers, 8 px, seed 0) with `kw` over them."""
    return L.make_opts(L.ResectOpts, "resectioning", **kw)


def _intr(intr):
    return np.ascontiguousarray(intr, np.float64).reshape(8)


def resect_images_csr(ids, corr_off, uv, world, intr, capacity=None, device=0, **opts):
    """(inliers int32 [n], inlier_off int64 [J + 1], report): the C call as it is.  `capacity` defaults to the number of
    correspondences, which no result can exceed; inlier_off holds the true offsets also where they pass a smaller capacity."""
    lib = L.load()
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    corr_off = np.ascontiguousarray(corr_off, np.int64)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 3)
    J = len(ids)
    if len(corr_off) != J + 1 or len(uv) != len(world):
        raise ValueError("corr_off must hold one offset per job and the total; uv and world one row per correspondence")
    if J and int(corr_off[-1]) != len(uv):
        raise ValueError("corr_off must end at the number of correspondences")
    intr = _intr(intr)
    o = resect_opts(lib, **opts)
    cap = int(len(uv) if capacity is None else capacity)
    inliers = np.zeros(max(cap, 0), np.int32)
    off = np.zeros(J + 1, np.int64)
    R, t = np.zeros((J, 9)), np.zeros((J, 3))
    status, n_inl, best_h = (np.zeros(J, np.int32) for _ in range(3))
    rmse, info = np.zeros(J), np.zeros((J, 36))
    L.check(lib.lvba_resect_images(int(device), J, ids.ctypes.data, corr_off.ctypes.data, uv.ctypes.data, world.ctypes.data, intr.ctypes.data,
                                   C.byref(o), cap, off.ctypes.data, inliers.ctypes.data, R.ctypes.data, t.ctypes.data, status.ctypes.data,
                                   n_inl.ctypes.data, best_h.ctypes.data, rmse.ctypes.data, info.ctypes.data))
    report = dict(ids=ids, Rcw=R.reshape(J, 3, 3), tcw=t, status=status, n_inliers=n_inl, n_matches=np.diff(corr_off).astype(np.int64),
                  best_h=best_h, rmse_px=rmse, information=info.reshape(J, 6, 6))
    return inliers[:max(min(int(off[-1]), cap), 0)], off, report


def resect_images(uv, world, intr, ids=None, device=0, **opts):
    """(inliers, report): uv[j] = [m_j, 2] pixels and world[j] = [m_j, 3] world points of job j; ids default to 0 .. J - 1.
    inliers: one int32 array of positions per job, in job order (empty for a job that is not OK); report: a dict of arrays ids,
    Rcw [J, 3, 3], tcw [J, 3] (T_cam<-world), status, n_inliers, n_matches, best_h, rmse_px, information [J, 6, 6]."""
    fu, off = L.flatten_rows(uv, np.float32, 2)
    fw, off_w = L.flatten_rows(world, np.float64, 3)
    if not np.array_equal(off, off_w):
        raise ValueError("uv and world must give the same number of rows per job")
    ids = np.arange(len(off) - 1, dtype=np.int32) if ids is None else ids
    inl, ioff, report = resect_images_csr(ids, off, fu, fw, intr, device=device, **opts)
    return [inl[ioff[j]:ioff[j + 1]] for j in range(len(ioff) - 1)], report


def hypotheses(job_id, uv, world, intr, device=0, **opts):
    """(R float64 [H, 3, 3], t [H, 3], count int32 [H]): every hypothesis of the job before the choice, without refinement; an
    invalid one has zeros and count = -1."""
    lib = L.load()
    o = resect_opts(lib, **opts)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 3)
    if len(uv) != len(world):
        raise ValueError("uv and world must hold one row per correspondence")
    intr = _intr(intr)
    H = max(int(o.hypotheses), 0)
    R, t, count = np.zeros((H, 9)), np.zeros((H, 3)), np.zeros(H, np.int32)
    L.check(lib.lvba_resect_hypotheses(int(device), int(job_id), len(uv), uv.ctypes.data, world.ctypes.data, intr.ctypes.data, C.byref(o),
                                       R.ctypes.data, t.ctypes.data, count.ctypes.data))
    return R.reshape(H, 3, 3), t, count


def score(uv, world, intr, Rcw, tcw, max_error_px=8.0, device=0):
    """bool [m]: which correspondences are inliers of the pose (Rcw, tcw) = T_cam<-world."""
    lib = L.load()
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 3)
    if len(uv) != len(world):
        raise ValueError("uv and world must hold one row per correspondence")
    intr = _intr(intr)
    R, t = np.ascontiguousarray(Rcw, np.float64).reshape(9), np.ascontiguousarray(tcw, np.float64).reshape(3)
    mask = np.zeros(len(uv), np.uint8)
    L.check(lib.lvba_resect_score(int(device), len(uv), uv.ctypes.data, world.ctypes.data, intr.ctypes.data, R.ctypes.data, t.ctypes.data,
                                  float(max_error_px), mask.ctypes.data))
    return mask.astype(bool)


def lift_keypoints(depth, keypoints, intr, Rcw, tcw):
    """One float64 [n_i, 3] array per image: the world point of every keypoint through the image's depth image (depth: a
    visual.DepthImages rendered or uploaded at the poses Rcw, tcw = T_cam<-world), NaN rows where a keypoint has none."""
    lib = L.load()
    uv, off = L.flatten_rows(keypoints, np.float32, 2)
    M = len(off) - 1
    intr = _intr(intr)
    R = np.ascontiguousarray(Rcw, np.float64).reshape(M, 9)
    t = np.ascontiguousarray(tcw, np.float64).reshape(M, 3)
    world = np.zeros((int(off[-1]), 3))
    L.check(lib.lvba_resect_lift(depth._h, M, off.ctypes.data, uv.ctypes.data, intr.ctypes.data, R.ctypes.data, t.ctypes.data, world.ctypes.data))
    return [world[off[i]:off[i + 1]] for i in range(M)]


def pose_offset(R, t, R2, t2):
    """(rotation angle in degrees, distance of the camera centres) between two poses T_cam<-world"""
    R, R2 = np.asarray(R, np.float64).reshape(3, 3), np.asarray(R2, np.float64).reshape(3, 3)
    c = 0.5 * (np.trace(R @ R2.T) - 1.0)
    ang = float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    return ang, float(np.linalg.norm(R.T @ np.asarray(t, np.float64).reshape(3) - R2.T @ np.asarray(t2, np.float64).reshape(3)))


def summary(report, Rcw=None, tcw=None):
    """The report as plain Python, for a JSON file: per image the status, the counts and the rmse -- and, given the poses Rcw, tcw
    the images were expected at, the rotation angle (degrees) and the distance of the camera centres between the resected and the
    given pose -- plus the totals and the medians over the OK images."""
    per = []
    for j in range(len(report["status"])):
        e = dict(image=int(report["ids"][j]), status=STATUS_NAMES[int(report["status"][j])], n_matches=int(report["n_matches"][j]),
                 n_inliers=int(report["n_inliers"][j]), rmse_px=float(report["rmse_px"][j]))
        if Rcw is not None and int(report["status"][j]) == OK:
            a, d = pose_offset(report["Rcw"][j], report["tcw"][j], np.asarray(Rcw).reshape(-1, 9)[j], np.asarray(tcw).reshape(-1, 3)[j])
            e.update(rotation_deg=a, translation=d)
        per.append(e)
    ok = [e for e in per if e["status"] == "ok"]
    out = dict(images=per, n_images=len(per), n_images_ok=len(ok))
    if Rcw is not None:
        out["median_rotation_deg"] = float(np.median([e["rotation_deg"] for e in ok])) if ok else None
        out["median_translation"] = float(np.median([e["translation"] for e in ok])) if ok else None
    return out
