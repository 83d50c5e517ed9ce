"""Descriptor matching of image pairs on the GPU, with an optional pose-guided gate -- on the epipolar line, or at the point a
LiDAR depth image predicts (lvba_match_*; the rule is in include/lvba_hip.h).  Opt-in: nothing imports this module unless matching is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.MatchOpts)


def match_opts(lib=None, **kw):
    """lvba_match_opts: the defaults (0.7, 0.8, mutual, unguided, 4 px, 8 px) with `kw` over them."""
    return L.make_opts(L.MatchOpts, "matching", **kw)


class Matcher(L.Handle):
    """The descriptors of a set of images resident on a GPU.  descriptors: a sequence of uint8 [n_i, 128] arrays."""
    _destroy = "lvba_match_destroy"

    def __init__(self, descriptors, device=0):
        self.lib = L.load()
        descs = []
        for d in descriptors:
            d = np.asarray(d)
            if d.size == 0:
                d = np.zeros((0, 128), np.uint8)
            if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 128:
                raise ValueError("each image's descriptors must be uint8 [n, 128]")
            descs.append(d)
        flat, self.off = L.flatten_rows(descs, np.uint8, 128)
        self.n_images = len(descs)
        self.counts = np.diff(self.off)
        self.device = int(device)
        self.has_geometry = False
        self.has_depth = False
        self._h = C.c_void_p()
        L.check(self.lib.lvba_match_create(self.device, self.n_images, self.off.ctypes.data, flat.ctypes.data, C.byref(self._h)))

    def set_geometry(self, keypoints, intr, Rcw, tcw):
        """keypoints: per image [n_i, 2] pixels (rounded to fp32), in descriptor order; intr (fx, fy, cx, cy, k1, k2, p1, p2);
        Rcw [M, 3, 3], tcw [M, 3] = T_cam<-world.  May be called again with new poses; the points of set_depth are dropped then
        (they were lifted with the old poses)."""
        uv, off = L.flatten_rows(keypoints, np.float32, 2)
        if not np.array_equal(off, self.off):
            raise ValueError("keypoints must give one [n_i, 2] array per image, a row per descriptor")
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        R = np.ascontiguousarray(Rcw, np.float64).reshape(self.n_images, 9)
        t = np.ascontiguousarray(tcw, np.float64).reshape(self.n_images, 3)
        L.check(self.lib.lvba_match_set_geometry(self._h, uv.ctypes.data, intr.ctypes.data, R.ctypes.data, t.ctypes.data))
        self.has_geometry = True
        self.has_depth = False

    def set_depth(self, depth):
        """depth: a visual.DepthImages with one image per image of the matcher, on its device (rendered at the poses of
        set_geometry), or None to drop the points.  Every keypoint with a depth return is lifted to its 3-D point once, on the
        device; guided=2 then gates a candidate at the point's image in the other view.  The depth set is only read during the
        call."""
        L.check(self.lib.lvba_match_set_depth(self._h, depth._h if depth is not None else None))
        self.has_depth = depth is not None

    def points(self):
        """float64 [total, 3]: the lifted point of every keypoint, image after image; NaN rows have none."""
        out = np.zeros((int(self.off[-1]), 3))
        L.check(self.lib.lvba_match_points(self._h, out.ctypes.data))
        return out

    def match_pairs_csr(self, pairs, capacity=None, **opts):
        """(matches int32 [m, 2], scores int32 [m], match_off int64 [n_pairs + 1], count): the C call as it is.  `capacity`
        defaults to a bound no pair can exceed."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        o = match_opts(self.lib, **opts)
        if capacity is None:
            ok = ((pairs >= 0) & (pairs < self.n_images)).all(axis=1) if len(pairs) else np.zeros(0, bool)
            na = self.counts[pairs[ok, 0]]
            capacity = int((np.minimum(na, self.counts[pairs[ok, 1]]) if o.mutual else na).sum())
        matches = np.zeros((int(capacity), 2), np.int32)
        scores = np.zeros(int(capacity), np.int32)
        off = np.zeros(len(pairs) + 1, np.int64)
        count = C.c_int64(0)
        L.check(self.lib.lvba_match_pairs(self._h, len(pairs), pairs.ctypes.data, C.byref(o), int(capacity), matches.ctypes.data,
                                          scores.ctypes.data, off.ctypes.data, C.byref(count)))
        m = min(int(count.value), int(capacity))
        return matches[:m], scores[:m], off, int(count.value)

    def match_pairs(self, pairs, return_scores=False, **opts):
        """One int32 [m, 2] array of (row in a, row in b) per pair, by ascending row; a pair without matches gives an empty array."""
        matches, scores, off, _ = self.match_pairs_csr(pairs, **opts)
        out = [matches[off[p]:off[p + 1]] for p in range(len(off) - 1)]
        if return_scores:
            return out, [scores[off[p]:off[p + 1]] for p in range(len(off) - 1)]
        return out

    def scan(self, a, b, **opts):
        """(best, s1, s2) int32 [n_a]: the raw top two of every row of the ordered pair (a, b), before any threshold."""
        o = match_opts(self.lib, **opts)
        n = int(self.counts[a]) if 0 <= int(a) < self.n_images else 0
        best, s1, s2 = (np.zeros(n, np.int32) for _ in range(3))
        L.check(self.lib.lvba_match_scan(self._h, int(a), int(b), C.byref(o), best.ctypes.data, s1.ctypes.data, s2.ctypes.data))
        return best, s1, s2


def match_pairs(descriptors, pairs, keypoints=None, intr=None, Rcw=None, tcw=None, device=0, depth=None, **opts):
    """Matcher(descriptors).match_pairs(pairs) in one call; guided when the geometry is given, depth-guided when a
    visual.DepthImages comes with it (unless guided is passed)."""
    with Matcher(descriptors, device=device) as m:
        if Rcw is not None:
            m.set_geometry(keypoints, intr, Rcw, tcw)
            opts.setdefault("guided", 1 if depth is None else 2)
            if depth is not None:
                m.set_depth(depth)
        elif depth is not None:
            raise ValueError("depth-guided matching needs the geometry (keypoints, intr, Rcw, tcw)")
        return m.match_pairs(pairs, **opts)
