"""LiDAR-camera extrinsic refinement on the GPU: T_cam<-imu from matches whose partner keypoint has a LiDAR depth, by Gauss-Newton
over all records at once, with the directions the trajectory leaves unobservable held (lvba_calib_*; the rule is in
include/lvba_hip.h).  Opt-in: nothing imports this module unless the refinement is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.CalibOpts)
CONVERGED, MAX_ITERATIONS, TOO_FEW_RECORDS, DEGENERATE = 0, 1, 2, 3
TD_OUT_OF_RANGE = 4
STATUS_NAMES = ("converged", "max_iterations", "too_few_records", "degenerate", "td_out_of_range")
TD_OPTION_NAMES = L.option_names(L.CalibTdOpts)


def calib_opts(**kw):
    """lvba_calib_opts: the defaults (20 iterations, Huber at 2 px -- the prototype's value, not tuned on data --, 100 records, no
    gate, min_eig_ratio 1e-6, eps 1e-10 rad / 1e-10 m) with `kw` over them.  loss_kind takes a name of _lib.LOSS_KINDS too."""
    if isinstance(kw.get("loss_kind"), str):
        kind = L.LOSS_KINDS.get(kw["loss_kind"].lower())
        if kind is None:
            raise ValueError(f"unknown loss kind {kw['loss_kind']!r}; one of {sorted(L.LOSS_KINDS)}")
        kw = dict(kw, loss_kind=kind)
    return L.make_opts(L.CalibOpts, "calibration", **kw)


def _inputs(records, pairs, body_poses, intr, Rci, tci):
    pair = np.ascontiguousarray(records["pair"], np.int32).reshape(-1)
    uv = np.ascontiguousarray(records["uv"], np.float32).reshape(-1, 2)
    Xb = np.ascontiguousarray(records["Xb"], np.float64).reshape(-1, 3)
    if not len(pair) == len(uv) == len(Xb):
        raise ValueError("records: pair, uv and Xb must hold one row per record")
    img_a, img_b = (np.ascontiguousarray(p, np.int32).reshape(-1) for p in pairs)
    if len(img_a) != len(img_b):
        raise ValueError("pairs: img_a and img_b must hold one entry per pair")
    poses = np.ascontiguousarray(body_poses, np.float64).reshape(-1, 12)
    intr = np.ascontiguousarray(intr, np.float64).reshape(8)
    R = np.ascontiguousarray(Rci, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(tci, np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError("one initial rotation and one initial translation per job")
    keep = (pair, uv, Xb, img_a, img_b, poses, intr, R, t)
    head = (len(poses), poses.ctypes.data, intr.ctypes.data, len(img_a), img_a.ctypes.data, img_b.ctypes.data, len(pair), pair.ctypes.data,
            uv.ctypes.data, Xb.ctypes.data, len(R), R.ctypes.data, t.ctypes.data)
    return keep, head, len(R)


def refine_jobs(records, pairs, body_poses, intr, Rci, tci, device=0, **opts):
    """The C call as it is: Rci [J, 3, 3] and tci [J, 3] are J initial extrinsics over the same records.  records: a dict of pair
    int32 [n], uv float32 [n, 2] (the keypoint in the pair's image a), Xb float64 [n, 3] (its match's lifted point in the camera
    frame of image b), grouped by pair; pairs: (img_a, img_b); body_poses [M, 12] = T_world<-imu at the image times.  Returns a
    dict of arrays Rci [J, 3, 3], tci [J, 3], status, iterations, n_used, rmse_px, cost, n_held, eigenvalues [J, 6] (ascending),
    eigenvectors [J, 6, 6] (row k the vector of eigenvalue k, order (om, up)), information [J, 6, 6]."""
    lib = L.load()
    o = calib_opts(**opts)
    keep, head, J = _inputs(records, pairs, body_poses, intr, Rci, tci)
    R, t = np.zeros((J, 9)), np.zeros((J, 3))
    status, iters, n_held = (np.zeros(J, np.int32) for _ in range(3))
    n_used = np.zeros(J, np.int64)
    rmse, cost = np.zeros(J), np.zeros(J)
    eig, vec, info = np.zeros((J, 6)), np.zeros((J, 36)), np.zeros((J, 36))
    L.check(lib.lvba_calib_extrinsic(int(device), *head, C.byref(o), R.ctypes.data, t.ctypes.data, status.ctypes.data, iters.ctypes.data,
                                     n_used.ctypes.data, rmse.ctypes.data, cost.ctypes.data, n_held.ctypes.data, eig.ctypes.data,
                                     vec.ctypes.data, info.ctypes.data))
    del keep
    return dict(Rci=R.reshape(J, 3, 3), tci=t, status=status, iterations=iters, n_used=n_used, rmse_px=rmse, cost=cost, n_held=n_held,
                eigenvalues=eig, eigenvectors=vec.reshape(J, 6, 6), information=info.reshape(J, 6, 6))


def best_job(report):
    """The converged job of lowest cost, the lowest index of a tie; None when no job converged."""
    best = None
    for j in range(len(report["status"])):
        if int(report["status"][j]) == CONVERGED and (best is None or report["cost"][j] < report["cost"][best]):
            best = j
    return best


def refine_extrinsic(records, pairs, body_poses, intr, Rci, tci, starts=None, device=0, **opts):
    """(Rci [3, 3], tci [3], report): the extrinsic refined from (Rci, tci).  starts: None, or further initial extrinsics [(R, t),
    ...] run over the same records in the same call (multi-start); the converged job of lowest cost wins, the lowest index on a
    tie (job 0 is (Rci, tci)).  report: refine_jobs' arrays of the winning job -- of job 0 when none converged, whose extrinsic
    is then returned as it came out, the status saying why -- plus job = its index and jobs = the arrays of all jobs."""
    Rs = [np.asarray(Rci, np.float64).reshape(9)] + [np.asarray(R, np.float64).reshape(9) for R, _ in (starts or [])]
    ts = [np.asarray(tci, np.float64).reshape(3)] + [np.asarray(t, np.float64).reshape(3) for _, t in (starts or [])]
    jobs = refine_jobs(records, pairs, body_poses, intr, np.array(Rs), np.array(ts), device=device, **opts)
    j = best_job(jobs)
    j = 0 if j is None else j
    report = {k: v[j] for k, v in jobs.items()}
    report.update(job=j, jobs=jobs)
    return report["Rci"], report["tci"], report


def linearize(records, pairs, body_poses, intr, Rci, tci, device=0, **opts):
    """(H [J, 6, 6], g [J, 6], cost [J], n_used int64 [J], sum_sq [J]): one evaluation of the rule at each of the J extrinsics, no
    step (the diagnostic call)."""
    lib = L.load()
    o = calib_opts(**opts)
    keep, head, J = _inputs(records, pairs, body_poses, intr, Rci, tci)
    H, g, cost, n_used, ssq = np.zeros((J, 36)), np.zeros((J, 6)), np.zeros(J), np.zeros(J, np.int64), np.zeros(J)
    L.check(lib.lvba_calib_linearize(int(device), *head, C.byref(o), H.ctypes.data, g.ctypes.data, cost.ctypes.data, n_used.ctypes.data,
                                     ssq.ctypes.data))
    del keep
    return H.reshape(J, 6, 6), g, cost, n_used, ssq


def summary(report, Rci, tci):
    """One job's report (refine_extrinsic's or refine_extrinsic_td's) as plain Python, for a JSON file: the status, the counts,
    the refined extrinsic, the rotation angle (degrees) and the translation distance between the given (Rci, tci) and the refined
    one, std_rot_deg and std_trans_m = the square roots of the traces of the rotation and translation blocks of rmse^2 H^+ (the
    pseudo-inverse over the free directions), and held = the held directions as (om, up) vectors in the camera frame -- (om, up,
    td) on the 7-parameter path, where time_offset_s is the refined offset and std_td_s the square root of the last diagonal entry
    of the same rmse^2 H^+; both are None on the 6-parameter path."""
    R0, t0 = np.asarray(Rci, np.float64).reshape(3, 3), np.asarray(tci, np.float64).reshape(3)
    R1, t1 = np.asarray(report["Rci"], np.float64).reshape(3, 3), np.asarray(report["tci"], np.float64).reshape(3)
    n_held = int(report["n_held"])
    lam = np.asarray(report["eigenvalues"], np.float64)
    n = len(lam)
    V = np.asarray(report["eigenvectors"], np.float64).reshape(n, n)
    out = dict(status=STATUS_NAMES[int(report["status"])], iterations=int(report["iterations"]), n_used=int(report["n_used"]),
               rmse_px=float(report["rmse_px"]), cost=float(report["cost"]), n_held=n_held, Rci=R1.tolist(), tci=t1.tolist(),
               rotation_deg=float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(R1 @ R0.T) - 1.0), -1.0, 1.0)))),
               translation_m=float(np.linalg.norm(t1 - t0)), eigenvalues=lam.tolist(), held=V[:n_held].tolist(),
               std_rot_deg=None, std_trans_m=None, time_offset_s=float(report["td"]) if "td" in report else None, std_td_s=None)
    if int(report["status"]) in (CONVERGED, MAX_ITERATIONS) and n_held < n:
        free = V[n_held:]
        cov = float(report["rmse_px"]) ** 2 * (free.T / lam[n_held:]) @ free
        out["std_rot_deg"] = float(np.degrees(np.sqrt(np.trace(cov[:3, :3]))))
        out["std_trans_m"] = float(np.sqrt(np.trace(cov[3:6, 3:6])))
        if n == 7:
            out["std_td_s"] = float(np.sqrt(cov[6, 6]))
    return out


# ---- the time offset as a seventh parameter (lvba_calib_*_td; include/lvba_hip.h, DESIGN.md §10o "time offset")

def calib_td_opts(**kw):
    """lvba_calib_td_opts: calib_opts' options and defaults, plus eps_td_s (1e-10 s) and max_abs_td_s (0.2 s)."""
    o = L.make_opts(L.CalibTdOpts, "calibration", _also=OPTION_NAMES, **{k: v for k, v in kw.items() if k in TD_OPTION_NAMES})
    o.calib = calib_opts(**{k: v for k, v in kw.items() if k not in TD_OPTION_NAMES})
    return o


def shift_poses(body_poses, twists, td):
    """The motion rule in numpy: the body poses [M, 12] = T_world<-imu of images stamped t, at t + td, each under its own constant
    twist (om body-frame rad/s, v world-frame m/s) [M, 6]: R <- R C with C the Cayley map of td om -- an exact rotation about om
    by 2 atan(td |om| / 2) --, P <- P + td v."""
    T = np.array(body_poses, np.float64).reshape(-1, 12)
    tw = np.asarray(twists, np.float64).reshape(-1, 6)
    if len(T) != len(tw):
        raise ValueError("one twist per body pose")
    th = float(td) * tw[:, :3]
    K = np.zeros((len(T), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -th[:, 2], th[:, 1], th[:, 2], -th[:, 0], -th[:, 1], th[:, 0]
    s = 1.0 + 0.25 * (th * th).sum(axis=1)
    Cm = np.eye(3) + (K + 0.5 * K @ K) / s[:, None, None]
    T[:, :9] = (T[:, :9].reshape(-1, 3, 3) @ Cm).reshape(-1, 9)
    T[:, 9:] += float(td) * tw[:, 3:]
    return T


def _inputs_td(records, pairs, body_poses, twists, intr, Rci, tci, td0):
    keep, head, J = _inputs(records, pairs, body_poses, intr, Rci, tci)
    tw = np.ascontiguousarray(twists, np.float64).reshape(-1, 6)
    if len(tw) != head[0]:
        raise ValueError("one twist per body pose")
    td = np.asarray(td0, np.float64).reshape(-1)
    td = np.full(J, td[0]) if len(td) == 1 else np.ascontiguousarray(td)
    if len(td) != J:
        raise ValueError("one initial time offset per job")
    return (keep, tw, td), head[:2] + (tw.ctypes.data,) + head[2:] + (td.ctypes.data,), J


def refine_jobs_td(records, pairs, body_poses, twists, intr, Rci, tci, td0=0.0, device=0, **opts):
    """refine_jobs with the time offset td as a seventh parameter: twists [M, 6] (pipeline.body_twists), td0 a scalar or [J].
    Returns refine_jobs' arrays plus td [J]; eigenvalues [J, 7], eigenvectors [J, 7, 7] (order (om, up, td)), information [J, 7, 7]."""
    lib = L.load()
    o = calib_td_opts(**opts)
    keep, head, J = _inputs_td(records, pairs, body_poses, twists, intr, Rci, tci, td0)
    R, t, td = np.zeros((J, 9)), np.zeros((J, 3)), np.zeros(J)
    status, iters, n_held = (np.zeros(J, np.int32) for _ in range(3))
    n_used = np.zeros(J, np.int64)
    rmse, cost = np.zeros(J), np.zeros(J)
    eig, vec, info = np.zeros((J, 7)), np.zeros((J, 49)), np.zeros((J, 49))
    L.check(lib.lvba_calib_extrinsic_td(int(device), *head, C.byref(o), R.ctypes.data, t.ctypes.data, td.ctypes.data, status.ctypes.data,
                                        iters.ctypes.data, n_used.ctypes.data, rmse.ctypes.data, cost.ctypes.data, n_held.ctypes.data,
                                        eig.ctypes.data, vec.ctypes.data, info.ctypes.data))
    del keep
    return dict(Rci=R.reshape(J, 3, 3), tci=t, td=td, status=status, iterations=iters, n_used=n_used, rmse_px=rmse, cost=cost,
                n_held=n_held, eigenvalues=eig, eigenvectors=vec.reshape(J, 7, 7), information=info.reshape(J, 7, 7))


def refine_extrinsic_td(records, pairs, body_poses, twists, intr, Rci, tci, td0=0.0, starts=None, device=0, **opts):
    """(Rci [3, 3], tci [3], td, report): refine_extrinsic with the time offset.  starts: further (R, t) or (R, t, td) to run over
    the same records; a start without an offset takes td0."""
    starts = [tuple(st) + (td0,) * (3 - len(st)) for st in (starts or [])]
    Rs = [np.asarray(Rci, np.float64).reshape(9)] + [np.asarray(R, np.float64).reshape(9) for R, _, _ in starts]
    ts = [np.asarray(tci, np.float64).reshape(3)] + [np.asarray(t, np.float64).reshape(3) for _, t, _ in starts]
    tds = [float(td0)] + [float(td) for _, _, td in starts]
    jobs = refine_jobs_td(records, pairs, body_poses, twists, intr, np.array(Rs), np.array(ts), np.array(tds), device=device, **opts)
    j = best_job(jobs)
    j = 0 if j is None else j
    report = {k: v[j] for k, v in jobs.items()}
    report.update(job=j, jobs=jobs)
    return report["Rci"], report["tci"], float(report["td"]), report


def linearize_td(records, pairs, body_poses, twists, intr, Rci, tci, td0=0.0, device=0, **opts):
    """(H [J, 7, 7], g [J, 7], cost [J], n_used int64 [J], sum_sq [J]): one evaluation at each (Rci, tci, td0), no step."""
    lib = L.load()
    o = calib_td_opts(**opts)
    keep, head, J = _inputs_td(records, pairs, body_poses, twists, intr, Rci, tci, td0)
    H, g, cost, n_used, ssq = np.zeros((J, 49)), np.zeros((J, 7)), np.zeros(J), np.zeros(J, np.int64), np.zeros(J)
    L.check(lib.lvba_calib_linearize_td(int(device), *head, C.byref(o), H.ctypes.data, g.ctypes.data, cost.ctypes.data,
                                        n_used.ctypes.data, ssq.ctypes.data))
    del keep
    return H.reshape(J, 7, 7), g, cost, n_used, ssq
