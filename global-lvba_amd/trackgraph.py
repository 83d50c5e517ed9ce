"""Feature tracks on the GPU: the key point match graph, its connected components with the two size checks, and the BFS order of
every component that visual.fuse_tracks consumes (lvba_trackgraph_*; the rule is in include/lvba_hip.h).
Opt-in: nothing imports this module unless device tracks are asked for (pipeline.build_tracks_and_fuse(device_tracks=True))."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _ptr(a):
    return a.ctypes.data if a.size else None


class TrackGraph(L.Handle):
    """TrackGraph(n_keypoints | keypoints, pairs, matches, obser_thr=3, device=0).  The first argument is either the key point
    count of every image or the key points themselves ([n_i, >= 2] per image; their first two columns go to the device and
    orders(uv=True) gathers them).  pairs / matches as pipeline.build_components takes them: one int [m, 2] array per pair.
    The graph, its component table and the adjacency stay on the device until close()."""
    _destroy = "lvba_trackgraph_destroy"

    def __init__(self, keypoints, pairs, matches, obser_thr=3, device=0):
        lib = L.load()
        counts = len(keypoints) == 0 or np.ndim(keypoints[0]) == 0
        if counts:
            uv, kp_off = None, np.concatenate([[0], np.cumsum([int(k) for k in keypoints])]).astype(np.int64)
        else:
            uv, kp_off = L.flatten_rows([np.asarray(k, np.float32).reshape(len(k), -1)[:, :2] if len(k) else [] for k in keypoints], np.float32, 2)
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        flat, match_off = L.flatten_rows(matches, np.int32, 2)
        if len(match_off) - 1 != len(pr):
            raise ValueError(f"{len(pr)} pairs but {len(match_off) - 1} match arrays")
        h, info = C.c_void_p(), L.TrackGraphInfo()
        L.check(lib.lvba_trackgraph_create(device, len(kp_off) - 1, kp_off.ctypes.data, None if uv is None else _ptr(uv), len(pr), _ptr(pr),
                                           match_off.ctypes.data, _ptr(flat), int(obser_thr), C.byref(h), C.byref(info)))
        self._h, self.lib, self.has_uv = h, lib, uv is not None
        self.info = info.as_dict()
        self._sizes = None

    def components(self):
        """(comp_off int64 [C + 1], mem_img int32, mem_kp int32, comp_images int32 [C]): the members of every qualifying component in
        scan order, the components by their smallest member."""
        nc, no = self.info["n_components"], self.info["n_observations"]
        off, img, kp, images = np.zeros(nc + 1, np.int64), np.zeros(no, np.int32), np.zeros(no, np.int32), np.zeros(nc, np.int32)
        L.check(self.lib.lvba_trackgraph_components(self._h, off.ctypes.data, _ptr(img), _ptr(kp), _ptr(images)))
        self._sizes = np.diff(off)
        return off, img, kp, images

    def orders(self, comp=None, attempt=0, uv=False):
        """(obs_off, obs_img, obs_kp[, obs_uv]): the BFS order from member `attempt` of every component of `comp` (strictly ascending
        indices; None: all)."""
        if uv and not self.has_uv:
            raise ValueError("orders(uv=True) needs a TrackGraph made from the key points, not from their counts")
        if self._sizes is None:
            self.components()
        sel = None if comp is None else np.ascontiguousarray(comp, np.int64).reshape(-1)
        if sel is not None and len(sel) == 0:
            none = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
            return none + (np.zeros((0, 2), np.float32),) if uv else none
        n = self.info["n_components"] if sel is None else len(sel)
        inside = sel is None or (sel.min() >= 0 and sel.max() < len(self._sizes))
        total = int((self._sizes if sel is None else self._sizes[sel]).sum()) if inside else 0       # a refusal writes nothing
        off, img, kp = np.zeros(n + 1, np.int64), np.zeros(total, np.int32), np.zeros(total, np.int32)
        puv = np.zeros((total, 2), np.float32) if uv else None
        L.check(self.lib.lvba_trackgraph_orders(self._h, n, None if sel is None else sel.ctypes.data, int(attempt),
                                                 off.ctypes.data, _ptr(img), _ptr(kp), None if puv is None else (puv.ctypes.data if total else None)))
        return (off, img, kp, puv) if uv else (off, img, kp)
