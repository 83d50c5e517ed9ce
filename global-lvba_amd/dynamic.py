"""Moving objects in the LiDAR map by range-image visibility (lvba_dynamic_labels, lvba_scans_select):

    d = dynamic_labels(scans, poses)                       # {"n_points", "n_judged", "n_dynamic", "ms", "label", "n_free", "n_support"}
    static = static_scans(scans, d["label"])               # a voxel.Scans without the points labelled dynamic

A point of frame f is labelled dynamic when enough other frames of its window measured a clearly longer range in its
direction and in all neighbouring directions -- they saw through it (include/lvba_hip.h has the exact rule, DESIGN.md §10m the
rationale).  The defaults are this project's choice and are not tuned on real data.  Everything runs in liblvba_hip.so on the
GPU; this file packs arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTIONS = L.option_names(L.DynamicOpts)
SUMMARY = ("n_points", "n_judged", "n_dynamic")


def default_opts():
    return L.make_opts(L.DynamicOpts, "dynamic")


def _opts(opts):
    return L.make_opts(L.DynamicOpts, "dynamic", **opts)


def dynamic_labels(scans, poses, frame_begin=0, n_frames=None, per_point=True, **opts):
    """The labels of the points of frames [frame_begin, frame_begin + n_frames) of scans (a voxel.Scans) at poses [n_frames, 12]
    (R row-major | t, T_world<-body), in cloud order: label uint8 (1 = dynamic), n_free and n_support int32 (with per_point),
    the summary counts and ms = the device times of the images, the dilation and the votes, and the download.  opts:
    lvba_dynamic_opts' fields."""
    fb = int(frame_begin)
    nf = scans.n_frames - fb if n_frames is None else int(n_frames)
    x = np.ascontiguousarray(poses, np.float64).reshape(-1)
    if x.size != 12 * max(nf, 0):
        raise ValueError(f"{x.size // 12} poses for {nf} frames")
    n = int(np.asarray(scans.counts)[fb:fb + max(nf, 0)].sum()) if 0 <= fb and nf > 0 else 0
    arrays = {}
    if per_point:
        arrays = dict(label=np.zeros(n, np.uint8), n_free=np.zeros(n, np.int32), n_support=np.zeros(n, np.int32))
    ptr = [arrays[k].ctypes.data if per_point and n else None for k in ("label", "n_free", "n_support")]
    s = L.DynamicSummary()
    L.check(L.load().lvba_dynamic_labels(scans._h, x if x.size else np.zeros(1), fb, nf, C.byref(_opts(opts)), C.byref(s), *ptr))
    out = {f: getattr(s, f) for f in SUMMARY}
    out["ms"] = dict(zip(("images", "dilation", "votes", "download"), list(s.ms)))
    out.update(arrays)
    return out


def select_scans(scans, keep):
    """A new voxel.Scans on the same device: every frame keeps its points with keep != 0 (one entry per point of the whole set, in
    cloud order), in scan order."""
    from .voxel import Scans
    k = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(-1)
    total = int(np.asarray(scans.counts).sum())
    if k.size != total:
        raise ValueError(f"{k.size} mask entries for {total} points")
    h = C.c_void_p()
    L.check(L.load().lvba_scans_select(scans._h, k.ctypes.data if total else None, C.byref(h)))
    out = Scans._from_handle(h)
    out.device = getattr(scans, "device", 0)
    return out


def static_scans(scans, label):
    """The scan set without the points labelled dynamic (label: dynamic_labels' over ALL frames of scans)."""
    return select_scans(scans, np.asarray(label) == 0)
