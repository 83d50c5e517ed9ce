"""Photometric camera alignment against the coloured map (lvba_palign_*; the rule is in include/lvba_hip.h):

    ref16, valid = reference_from_sums(n_views, s1, min_views)        # from photo.PhotoMap.sums()
    with PhotoAligner(points, ref16, valid, n_images, width, height, intr, depth=depth_images) as pa:
        res = pa.linearize(first, Rcw, tcw, bgr)                     # dict(H, g, cost, n_samples, sum_sq, sum_w): no step
        out = pa.align(first, Rcw, tcw, bgr)                         # dict(Rcw, tcw, status, iterations, accepted, n_samples, ...)

The map's colours are held fixed and each camera is moved until its image agrees with them (Levenberg-Marquardt per image on the
per-channel colour residuals, the fusion's own samples and their bilinear gradient).  Everything runs in liblvba_hip.so on the GPU;
this file packs arrays.  Opt-in: nothing imports this module unless the stage is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.PalignOpts)
STATUS = {0: "CONVERGED", 1: "MAX_ITERATIONS", 2: "TOO_FEW_SAMPLES", 3: "DEGENERATE", 4: "OUT_OF_BOUNDS"}
CONVERGED, MAX_ITERATIONS, TOO_FEW_SAMPLES, DEGENERATE, OUT_OF_BOUNDS = range(5)
N_SUMS = 31


def palign_opts(**kw):
    """lvba_palign_opts: the defaults (the fusion's occlusion test, Huber at 10 grey levels, 200 samples, 15 passes, 5 degrees and
    0.5 m of reach; none tuned on recorded data) with `kw` over them."""
    return L.make_opts(L.PalignOpts, "photometric alignment", **kw)


def reference_from_sums(n_views, s1, min_views=2):
    """(ref16 uint16 [n, 3], valid uint8 [n]) from the fusion's integer sums: per channel (2 S1 + n_views) // (2 n_views), the
    round-half-up mean in 1/256 grey level; a point below min_views is invalid (reference 0)."""
    n = np.asarray(n_views, np.int64).reshape(-1)
    s = np.asarray(s1).astype(np.int64).reshape(-1, 3)
    valid = n >= max(int(min_views), 1)
    nn = np.where(valid, n, 1)[:, None]
    ref = np.where(valid[:, None], (2 * s + nn) // (2 * nn), 0)
    return np.ascontiguousarray(ref.astype(np.uint16)), np.ascontiguousarray(valid.astype(np.uint8))


def unpack_sums(sums):
    """dict(H [m, 6, 6], g [m, 6], cost, n_samples int64, sum_sq, sum_w [m]) of sums [m, 31]"""
    s = np.asarray(sums, np.float64).reshape(-1, N_SUMS)
    H = np.zeros((len(s), 6, 6))
    iu = np.triu_indices(6)
    H[:, iu[0], iu[1]] = s[:, :21]
    H[:, iu[1], iu[0]] = s[:, :21]
    return dict(H=H, g=s[:, 21:27].copy(), cost=s[:, 27].copy(), n_samples=s[:, 28].astype(np.int64), sum_sq=s[:, 29].copy(),
                sum_w=s[:, 30].copy())


class PhotoAligner(L.Handle):
    """`points` [n, 3] (float32 world points) with their reference colours ref16 [n, 3] (uint16; b, g, r in 1/256 grey level) and
    validity bytes valid [n], against n_images images of width x height through intr = fx fy cx cy k1 k2 p1 p2.  depth: a
    visual.DepthImages of the same images at the initial poses (the occlusion test), kept alive by the caller, or None."""
    _destroy = "lvba_palign_free"

    def __init__(self, points, ref16, valid, n_images, width, height, intr, depth=None, device=0, **opts):
        self.lib = L.load()
        xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(ref16, np.uint16).reshape(-1, 3)
        ok = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if len(ref) != len(xyz) or len(ok) != len(xyz):
            raise ValueError(f"{len(xyz)} points, {len(ref)} reference colours, {len(ok)} validity bytes")
        self.n, self.n_images, self.width, self.height = len(xyz), int(n_images), int(width), int(height)
        self.depth = depth
        o = palign_opts(**opts)
        self.options = {k: getattr(o, k) for k in OPTION_NAMES}
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_palign_create(int(device), self.n, xyz.ctypes.data, ref.ctypes.data, ok.ctypes.data, self.n_images, self.width,
                                            self.height, intr.ctypes.data, depth._h if depth is not None else None, C.byref(o),
                                            C.byref(self._h)))

    def _pack(self, Rcw, tcw, bgr):
        R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9)
        t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
        img = np.ascontiguousarray(bgr, np.uint8)
        m = len(R)
        if len(t) != m or img.shape != (m, self.height, self.width, 3):
            raise ValueError(f"{m} rotations, {len(t)} translations, bgr {img.shape} (want [{m}, {self.height}, {self.width}, 3])")
        return R, t, img, m

    def linearize(self, first, Rcw, tcw, bgr):
        """One evaluation of images first .. first + m - 1 at the given poses, no step: unpack_sums' dict with the raw "sums" [m, 31]."""
        R, t, img, m = self._pack(Rcw, tcw, bgr)
        sums = np.zeros((m, N_SUMS))
        L.check(self.lib.lvba_palign_linearize(self._h, int(first), m, R.ctypes.data, t.ctypes.data, img.ctypes.data, sums.ctypes.data))
        return dict(unpack_sums(sums), sums=sums)

    def align(self, first, Rcw, tcw, bgr):
        """The iteration on images first .. first + m - 1 from the given poses: dict(Rcw [m, 3, 3], tcw [m, 3], status, iterations,
        accepted int32 [m], n_samples int64 [m], rmse_initial, rmse, cost [m], information [m, 6, 6])."""
        R, t, img, m = self._pack(Rcw, tcw, bgr)
        out = dict(Rcw=np.zeros((m, 3, 3)), tcw=np.zeros((m, 3)), status=np.zeros(m, np.int32), iterations=np.zeros(m, np.int32),
                   accepted=np.zeros(m, np.int32), n_samples=np.zeros(m, np.int64), rmse_initial=np.zeros(m), rmse=np.zeros(m),
                   cost=np.zeros(m), information=np.zeros((m, 6, 6)))
        L.check(self.lib.lvba_palign_align(self._h, int(first), m, R.ctypes.data, t.ctypes.data, img.ctypes.data,
                                           *(out[k].ctypes.data for k in ("Rcw", "tcw", "status", "iterations", "accepted", "n_samples",
                                                                          "rmse_initial", "rmse", "cost", "information"))))
        return out

    def profile(self):
        """device ms of the uploads, the linearisation passes and the steps, accumulated over this handle's calls"""
        ms = np.zeros(3)
        L.check(self.lib.lvba_palign_profile(self._h, ms.ctypes.data))
        return dict(upload=float(ms[0]), linearize=float(ms[1]), step=float(ms[2]))
