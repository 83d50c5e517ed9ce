"""Scan-to-map registration (lvba_register_*): point-to-plane Gauss-Newton of scans against a voxel plane map.

    with scans.voxel_map(poses[:5], 1.0, STRICT_RATIO, n_frames=5) as m:
        r = m.register(scans, [5], poses[5:6])           # {"poses", "information", "status", "rmse", ...}

Every point of a scan is taken to the world by the job's pose, associated with the map's plane exactly as
VoxelMap.find_planes does it, and contributes its point-to-plane distance r if |r| <= max_distance; the pose is refined by
Gauss-Newton under the retraction R <- R Exp(theta), t <- t + delta (include/lvba_hip.h has the exact definitions).  Build the
map with strict eigen ratios (STRICT_RATIO) or set a loss: a map cut with the optimiser's stage-1 ratios admits planes fitted
through clutter, and plain Gauss-Newton walks away from the true pose on it.  A submap set (voxel.SubmapSet, Scans.submaps) holds many
submaps in one map: its register / linearize take a submap index per job.  loop_candidates finds which frame revisits which
submap from the poses alone; scan_descriptors / place_search / place_candidates find it from the clouds alone (Scan Context
descriptors: DESIGN.md §10e), with the relative yaw.  Everything runs in liblvba_hip.so on the GPU; this file packs arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

STRICT_RATIO = (0.02, 0.02, 0.02, 0.02)   # eigen ratios of a registration map
OPTS = L.option_names(L.RegisterOpts)          # `loss` is an option too: a (kind, scale) pair, see _opts


def default_opts():
    return L.make_opts(L.RegisterOpts, "registration")


def _opts(kw):
    kw = dict(kw)
    loss = kw.pop("loss", None)
    o = L.make_opts(L.RegisterOpts, "registration", ("loss",), **kw)
    if loss is not None:                    # None leaves the library's default
        o.loss = L.loss_struct(loss).contents
    return o


def _jobs(frames, poses):
    fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
    x = np.ascontiguousarray(poses, np.float64).reshape(-1)
    if x.size != 12 * len(fr):
        raise ValueError(f"{x.size // 12} poses for {len(fr)} frames")
    return fr, x


def _submap(submap, n):
    sm = np.ascontiguousarray(submap, np.int32).reshape(-1)
    if len(sm) != n:
        raise ValueError(f"{len(sm)} submap indices for {n} frames")
    return sm


def linearize(vmap, scans, frames, poses, submap=None, **opts):
    """The sums of one linearisation per job (lvba_register_linearize): dict(H [n,6,6], g [n,6], cost [n], inliers [n]).
    submap: None, or one submap index per job for a submap set (lvba_register_linearize_submaps)."""
    fr, x = _jobs(frames, poses)
    n = len(fr)
    H, g, cost, inl = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros(n), np.zeros(n, np.int64)
    o = _opts(opts)
    if submap is None:
        L.check(L.load().lvba_register_linearize(vmap._h, scans._h, n, fr.ctypes.data, x.ctypes.data, C.byref(o), H.ctypes.data,
                                                 g.ctypes.data, cost.ctypes.data, inl.ctypes.data))
    else:
        sm = _submap(submap, n)
        L.check(L.load().lvba_register_linearize_submaps(vmap._h, scans._h, n, fr.ctypes.data, sm.ctypes.data, x.ctypes.data, C.byref(o),
                                                         H.ctypes.data, g.ctypes.data, cost.ctypes.data, inl.ctypes.data))
    return dict(H=H, g=g, cost=cost, inliers=inl)


def register(vmap, scans, frames, poses, submap=None, **opts):
    """Register frame frames[k] of `scans` (a voxel.Scans) from poses[k] against `vmap` (a voxel.VoxelMap), all jobs at once
    (lvba_register_scans).  opts: max_iterations, max_distance [m], min_inliers, min_eigenvalue, tol_rot [rad], tol_pos [m],
    loss=(kind, scale [m]).  Returns dict(poses [n,12], information [n,6,6] (H of the last linearisation, tangent order
    (theta, t)), status [n] (a _lib.REG_STATUS key), status_name, iterations, inliers, points, cost_first, cost_last, rmse,
    min_eigenvalue).  submap: None, or one submap index per job for a submap set (lvba_register_scans_submaps)."""
    fr, x = _jobs(frames, poses)
    n = len(fr)
    out, info = np.zeros((n, 12)), np.zeros((n, 6, 6))
    res = (L.RegisterResult * max(n, 1))()
    o = _opts(opts)
    if submap is None:
        L.check(L.load().lvba_register_scans(vmap._h, scans._h, n, fr.ctypes.data, x.ctypes.data, C.byref(o), out.ctypes.data,
                                             info.ctypes.data, C.cast(res, C.c_void_p)))
    else:
        sm = _submap(submap, n)
        L.check(L.load().lvba_register_scans_submaps(vmap._h, scans._h, n, fr.ctypes.data, sm.ctypes.data, x.ctypes.data, C.byref(o),
                                                     out.ctypes.data, info.ctypes.data, C.cast(res, C.c_void_p)))
    d = dict(poses=out, information=info)
    for f, t in L.RegisterResult._fields_:
        d[f] = np.array([getattr(res[k], f) for k in range(n)], np.float64 if t is C.c_double else np.int64)
    d["status_name"] = [L.REG_STATUS.get(int(s), "?") for s in d["status"]]
    return d


LOOP_OPTS = L.option_names(L.LoopOpts)


def loop_candidates(poses, device=0, capacity=None, **opts):
    """Loop-closure candidates from the poses [n,12] alone (lvba_loop_candidates; include/lvba_hip.h has the exact rule): every
    query frame (a multiple of query_stride) against every submap of submap_size frames that lies at least min_gap frames away
    and comes within radius [m]; the max_per_frame nearest per query.  Returns dict(query, submap, ref (the submap's nearest
    frame), distance [m], count), sorted by (query, submap).  capacity: None (all of them), or the number of entries to fetch;
    count is the true number either way."""
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    o = L.make_opts(L.LoopOpts, "candidate", **opts)
    lib = L.load()
    count = C.c_int64()
    cap = len(x) * max(1, min(32, o.max_per_frame)) if capacity is None else int(capacity)
    buf = np.zeros(max(cap, 1), np.dtype([("query", "<i4"), ("submap", "<i4"), ("ref", "<i4"), ("pad", "<i4"), ("distance", "<f8")]))
    L.check(lib.lvba_loop_candidates(int(device), len(x), x.ctypes.data, C.byref(o), cap, buf.ctypes.data, C.byref(count)))
    got = buf[:min(cap, count.value)]
    return dict(query=got["query"].copy(), submap=got["submap"].copy(), ref=got["ref"].copy(), distance=got["distance"].copy(),
                count=count.value, raw=got.copy())


PLACE_OPTS = L.option_names(L.PlaceOpts)
PLACE_DTYPE = np.dtype([("query", "<i4"), ("submap", "<i4"), ("ref", "<i4"), ("shift", "<i4"), ("distance", "<f8"), ("yaw", "<f8")])


def _place_opts(opts):
    return L.make_opts(L.PlaceOpts, "place", **opts)


def _place_result(call, n, o, capacity):
    count = C.c_int64()
    cap = n * max(1, min(32, o.max_per_frame)) if capacity is None else int(capacity)
    buf = np.zeros(max(cap, 1), PLACE_DTYPE)
    L.check(call(C.byref(o), cap, buf.ctypes.data, C.byref(count)))
    got = buf[:min(cap, count.value)]
    d = {k: got[k].copy() for k in PLACE_DTYPE.names}
    d.update(count=count.value, raw=got.copy())
    return d


def scan_descriptors(scans, frame_begin=0, n_frames=None, **opts):
    """Scan Context descriptors of frames [frame_begin, frame_begin + n_frames) of `scans` (a voxel.Scans; default: to the last
    frame): (desc [n, n_rings, n_sectors] float32, ring_key [n, n_rings] float32) -- lvba_place_descriptors; include/lvba_hip.h
    has the exact rule.  opts: n_rings, n_sectors, min_range, max_range, z_offset (the others of PLACE_OPTS are accepted and
    have no bearing on a descriptor)."""
    o = _place_opts(opts)
    n = scans.n_frames - int(frame_begin) if n_frames is None else int(n_frames)
    desc, key = np.zeros((max(n, 0), o.n_rings, o.n_sectors), np.float32), np.zeros((max(n, 0), o.n_rings), np.float32)
    L.check(L.load().lvba_place_descriptors(scans._h, int(frame_begin), n, C.byref(o), desc.ctypes.data, key.ctypes.data))
    return desc, key


def place_search(desc, device=0, capacity=None, **opts):
    """Place-recognition candidates among descriptors desc [n, n_rings, n_sectors] from anywhere (lvba_place_search): per query
    frame the n_key_candidates frames of the nearest ring keys, at least min_gap frames away, get the column-shift distance; per
    submap the best frame is ref; the max_per_frame submaps within max_distance are kept.  Returns dict(query, submap, ref,
    shift, distance, yaw [rad, the query's body is ref's turned by yaw about z], count, raw), sorted by (query, submap).
    n_rings / n_sectors default to desc's shape.  capacity: as loop_candidates."""
    d = np.ascontiguousarray(desc, np.float32)
    if d.ndim != 3:
        raise ValueError("desc must be [n, n_rings, n_sectors]")
    o = _place_opts(dict(dict(n_rings=d.shape[1], n_sectors=d.shape[2]), **opts))
    if (o.n_rings, o.n_sectors) != d.shape[1:]:
        raise ValueError(f"desc is {d.shape[1]} x {d.shape[2]}, the options say {o.n_rings} x {o.n_sectors}")
    lib = L.load()
    return _place_result(lambda po, cap, out, cnt: lib.lvba_place_search(int(device), len(d), d.ctypes.data, po, cap, out, cnt), len(d), o, capacity)


def place_candidates(scans, capacity=None, **opts):
    """place_search over the descriptors of all frames of `scans`, the descriptors never leaving the device
    (lvba_place_candidates): the same bytes as scan_descriptors followed by place_search."""
    o = _place_opts(opts)
    lib = L.load()
    return _place_result(lambda po, cap, out, cnt: lib.lvba_place_candidates(scans._h, po, cap, out, cnt), scans.n_frames, o, capacity)


CLOSURE_OPTS = L.option_names(L.ClosureOpts)


def closure_consistency(poses, ref, query, meas, device=0, diagnostics=False, **opts):
    """Pairwise consistency of loop closures (lvba_closure_consistency; include/lvba_hip.h has the exact rule, after Mangelson et
    al., PCM, ICRA 2018): closure k measures meas[k] = T_ref^-1 T_query (12 numbers, R row-major | t); every pair of closures is
    tested against the relative motion of the current `poses` [n_frames,12] between them, and a large mutually consistent set is
    kept by a greedy search from n_seeds seeds (not guaranteed to be the largest).  opts: rot_tol [rad], rot_rate [rad per frame],
    trans_tol [m], trans_rate [m per frame], n_seeds, min_set.  Returns dict(keep bool [n], n_keep, adjacency bool [n,n], words
    uint64 [n, ceil(n/64)] as the library lays the adjacency out) and, with diagnostics=True, rot / trans [n,n] (the two measures
    of every cycle; n * n doubles each)."""
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    z = np.ascontiguousarray(meas, np.float64).reshape(-1, 12)
    i, j = np.ascontiguousarray(ref, np.int32).reshape(-1), np.ascontiguousarray(query, np.int32).reshape(-1)
    n = len(z)
    if len(i) != n or len(j) != n:
        raise ValueError(f"{n} measurements for {len(i)} ref and {len(j)} query frames")
    o = L.make_opts(L.ClosureOpts, "closure", **opts)
    lib = L.load()
    W = (n + 63) // 64
    words, keep, n_keep = np.zeros((n, W), np.uint64), np.zeros(n, np.uint8), C.c_int32()
    rot, trans = (np.zeros((n, n)), np.zeros((n, n))) if diagnostics else (None, None)
    L.check(lib.lvba_closure_consistency(int(device), len(x), x.ctypes.data, n, i.ctypes.data, j.ctypes.data, z.ctypes.data, C.byref(o),
                                         words.ctypes.data, rot.ctypes.data if diagnostics else None,
                                         trans.ctypes.data if diagnostics else None, keep.ctypes.data, C.byref(n_keep)))
    adj = np.unpackbits(words.view(np.uint8).reshape(n, 8 * W), axis=1, bitorder="little")[:, :n].astype(bool) if n else np.zeros((0, 0), bool)
    d = dict(keep=keep.astype(bool), n_keep=int(n_keep.value), adjacency=adj, words=words)
    if diagnostics:
        d.update(rot=rot, trans=trans)
    return d
