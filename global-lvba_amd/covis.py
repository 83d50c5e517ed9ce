"""Which image pairs to match, from LiDAR co-visibility on the GPU: a grid of samples per image lifted through the image's own depth
image, projected into every other image and tested against that image's depth for occlusion (lvba_covis_*; the rule is in
include/lvba_hip.h).  Opt-in: nothing imports this module unless pair selection is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.CovisOpts)
INT_OPTIONS = tuple(f for f, t in L.CovisOpts._fields_ if f in OPTION_NAMES and t is C.c_int32)
FLOAT_OPTIONS = tuple(f for f in OPTION_NAMES if f not in INT_OPTIONS)


def covis_opts(lib=None, **kw):
    """lvba_covis_opts: the defaults (a 16 x 12 grid, radius 4, occlusion on at 5 % + 0.1 m, either way, no cap, 8 samples,
    overlap 0.1) with `kw` over them."""
    return L.make_opts(L.CovisOpts, "pair selection", **kw)


def _geometry(depth, Rcw, tcw, intr):
    M = depth.n_images
    R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
    if len(R) != M or len(t) != M:
        raise ValueError(f"{M} depth images but {len(R)} rotations and {len(t)} translations")
    return M, R, t, np.ascontiguousarray(intr, np.float64).reshape(8)


def samples(depth, Rcw, tcw, intr, **opts):
    """float64 [M, G, 3]: the world point of every grid cell of every image, NaN rows where a cell has none.  depth: a
    visual.DepthImages; Rcw [M, 3, 3], tcw [M, 3] = T_cam<-world; intr (fx, fy, cx, cy, k1, k2, p1, p2)."""
    lib = L.load()
    M, R, t, intr = _geometry(depth, Rcw, tcw, intr)
    o = covis_opts(lib, **opts)
    out = np.zeros((M, o.grid_x * o.grid_y, 3))
    L.check(lib.lvba_covis_samples(depth._h, R.ctypes.data, t.ctypes.data, intr.ctypes.data, C.byref(o), out.ctypes.data))
    return out


def counts(depth, Rcw, tcw, intr, **opts):
    """(n_points int32 [M]: the cells of each image with a point, counts int32 [M, M]: the samples of image i seen in image j)"""
    lib = L.load()
    M, R, t, intr = _geometry(depth, Rcw, tcw, intr)
    o = covis_opts(lib, **opts)
    n, c = np.zeros(M, np.int32), np.zeros((M, M), np.int32)
    L.check(lib.lvba_covis_counts(depth._h, R.ctypes.data, t.ctypes.data, intr.ctypes.data, C.byref(o), n.ctypes.data, c.ctypes.data))
    return n, c


def select_pairs(depth, Rcw, tcw, intr, capacity=None, **opts):
    """(pairs int32 [m, 2] with i < j sorted by (i, j), score float64 [m], shared int32 [m, 2] = (c_ij, c_ji)).  `capacity`
    defaults to a guess of 16 pairs per image; when the selection is larger the call is made once more with room for all."""
    lib = L.load()
    M, R, t, intr = _geometry(depth, Rcw, tcw, intr)
    o = covis_opts(lib, **opts)
    cap = min(M * (M - 1) // 2, 16 * M) if capacity is None else int(capacity)
    for _ in range(2):
        pairs, score, shared = np.zeros((cap, 2), np.int32), np.zeros(cap), np.zeros((cap, 2), np.int32)
        count = C.c_int64(0)
        L.check(lib.lvba_covis_pairs(depth._h, R.ctypes.data, t.ctypes.data, intr.ctypes.data, C.byref(o), cap, pairs.ctypes.data,
                                     score.ctypes.data, shared.ctypes.data, C.byref(count)))
        if count.value <= cap:
            break
        cap = int(count.value)
    m = int(count.value)
    return pairs[:m], score[:m], shared[:m]
