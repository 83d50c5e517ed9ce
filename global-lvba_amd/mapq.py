"""Map quality without ground truth (lvba_mapq_*): the mean map entropy (MME) and mean plane variance (MPV) of Razlaw et al.
2015 over the aggregated LiDAR cloud, with per-point entropy, plane variance, normal and neighbour count on request:

    q = map_quality_scans(scans, poses)                    # {"mme": ..., "mpv": ..., "n_valid": ..., ...}
    q = map_quality_points(xyz, per_point=True)            # + "entropy", "plane_var", "normal", "count"

For every query point the neighbours within `radius` give a covariance S; entropy = 1/2 ln det(2 pi e S), plane_var = its
smallest eigenvalue (include/lvba_hip.h has the exact definitions).  A sharper map has a lower MME, whatever voxel size the
optimiser used.  Everything runs in liblvba_hip.so on the GPU; this file packs arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _opts(radius, min_neighbors, query_stride):
    return L.make_opts(L.MapqOpts, "map quality", radius=radius, min_neighbors=min_neighbors, query_stride=query_stride)


def _call(fn, head, n_points, o, per_point):
    s = L.MapqSummary()
    nq = -(-int(n_points) // max(1, o.query_stride))
    arrays = {}
    if per_point:
        arrays = dict(entropy=np.zeros(nq), plane_var=np.zeros(nq), normal=np.zeros((nq, 3), np.float32), count=np.zeros(nq, np.int32))
    ptr = [arrays[k].ctypes.data if per_point and nq else None for k in ("entropy", "plane_var", "normal", "count")]
    L.check(fn(*head, C.byref(o), C.byref(s), *ptr))
    out = {f: getattr(s, f) for f in ("n_points", "n_queries", "n_valid", "mme", "mpv", "mean_neighbors")}
    out["ms"] = dict(zip(("world", "sort", "reduce", "download"), list(s.ms)))
    out.update(arrays)
    return out


def map_quality_scans(scans, poses, radius=0.3, min_neighbors=8, query_stride=1, frame_begin=0, n_frames=None, per_point=False):
    """The metrics of frames [frame_begin, frame_begin + n_frames) of scans (a voxel.Scans) at poses [n_frames, 12] (R row-major
    | t, T_world<-body).  Every query_stride-th point of the cloud is a query; the neighbours are always all points."""
    fb = int(frame_begin)
    nf = scans.n_frames - fb if n_frames is None else int(n_frames)
    x = np.ascontiguousarray(poses, np.float64).reshape(-1)
    if x.size != 12 * max(nf, 0):
        raise ValueError(f"{x.size // 12} poses for {nf} frames")
    n_points = int(np.asarray(scans.counts)[fb:fb + max(nf, 0)].sum()) if 0 <= fb and nf > 0 else 0
    return _call(L.load().lvba_mapq_scans, (scans._h, x if x.size else np.zeros(1), fb, nf), n_points,
                 _opts(radius, min_neighbors, query_stride), per_point)


def map_quality_points(xyz, radius=0.3, min_neighbors=8, query_stride=1, per_point=False, device=0):
    """The metrics of a cloud xyz [n, 3] (stored as float32), e.g. ColorMap.download()[0]."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return _call(L.load().lvba_mapq_points, (int(device), len(p), p.ctypes.data if len(p) else None), len(p),
                 _opts(radius, min_neighbors, query_stride), per_point)
