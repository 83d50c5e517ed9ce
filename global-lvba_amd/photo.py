"""Multi-view colour fusion and photometric consistency of the map (lvba_photo_*; the rule is in include/lvba_hip.h):

    with PhotoMap(points, n_images, intr, width, height, depth=depth_images) as pm:
        pm.add_images(first, Rcw, tcw, bgr)               # any number of calls, each image index at most once
        out = pm.finish()                                 # dict(summary, n_views, rgb, sigma)

Every point is projected into every image that sees it, with the co-visibility stage's occlusion test against the depth images;
the colour is sampled there; `rgb` is the mean over the views and `sigma` their spread in grey levels.  summary["mean_sigma"]
drops when cameras, extrinsic and trajectory agree with the images.  Everything runs in liblvba_hip.so on the GPU; this file
packs arrays.  Opt-in: nothing imports this module unless the measure is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.PhotoOpts)


def photo_opts(**kw):
    """lvba_photo_opts: the defaults (occlusion at 5 % + 0.1 m, no depth limit, a sample needs a depth return, two views, batches
    by the free memory; none tuned on recorded data) with `kw` over them."""
    return L.make_opts(L.PhotoOpts, "photometric consistency", **kw)


class PhotoMap(L.Handle):
    """The running sums of `points` [n, 3] (float32 world points) over n_images images of width x height through intr = fx fy cx cy
    k1 k2 p1 p2.  depth: a visual.DepthImages of the same images (the occlusion test), kept alive by the caller, or None."""
    _destroy = "lvba_photo_free"

    def __init__(self, points, n_images, intr, width, height, depth=None, device=0, **opts):
        self.lib = L.load()
        xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.n, self.n_images, self.width, self.height = len(xyz), int(n_images), int(width), int(height)
        self.depth = depth
        o = photo_opts(**opts)
        self.options = {k: getattr(o, k) for k in OPTION_NAMES}
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_photo_create(int(device), self.n, xyz.ctypes.data, self.n_images, self.width, self.height, intr.ctypes.data,
                                           depth._h if depth is not None else None, C.byref(o), C.byref(self._h)))

    def add_images(self, first, Rcw, tcw, bgr, gains=None):
        """images first .. first + m - 1: Rcw [m, 3, 3], tcw [m, 3] (T_cam<-world); bgr [m, height, width, 3] uint8.  gains: None, or
        the exposure gains int64 [m, 3, 2] of these images (expo.estimate_exposure), applied to every sample."""
        R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9)
        t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
        img = np.ascontiguousarray(bgr, np.uint8)
        m = len(R)
        if len(t) != m or img.shape != (m, self.height, self.width, 3):
            raise ValueError(f"{m} rotations, {len(t)} translations, bgr {img.shape} (want [{m}, {self.height}, {self.width}, 3])")
        if gains is None:                        # (the plain entry point: lvba_photo_add_images_gains is not looked up)
            L.check(self.lib.lvba_photo_add_images(self._h, int(first), m, R.ctypes.data, t.ctypes.data, img.ctypes.data))
            return
        g = np.ascontiguousarray(gains, np.int64)
        if g.shape != (m, 3, 2):
            raise ValueError(f"gains {g.shape} (want [{m}, 3, 2])")
        L.check(self.lib.lvba_photo_add_images_gains(self._h, int(first), m, R.ctypes.data, t.ctypes.data, img.ctypes.data, g.ctypes.data))

    def finish(self):
        """dict(summary, n_views int32 [n], rgb uint8 [n, 3], sigma float64 [n]: NaN below min_views) of the images added so far"""
        s = L.PhotoSummary()
        nv, rgb, sigma = np.zeros(self.n, np.int32), np.zeros((self.n, 3), np.uint8), np.zeros(self.n)
        L.check(self.lib.lvba_photo_finish(self._h, C.byref(s), nv.ctypes.data, rgb.ctypes.data, sigma.ctypes.data))
        return dict(summary=s.as_dict(), n_views=nv, rgb=rgb, sigma=sigma)

    def sums(self):
        """(n_views int32 [n], s1 uint32 [n, 3], s2 int64 [n, 3]): the integer sums, channels b, g, r"""
        nv, s1, s2 = np.zeros(self.n, np.int32), np.zeros((self.n, 3), np.uint32), np.zeros((self.n, 3), np.int64)
        L.check(self.lib.lvba_photo_sums(self._h, nv.ctypes.data, s1.ctypes.data, s2.ctypes.data))
        return nv, s1, s2


def photo_consistency(points, images, Rcw, tcw, intr, width, height, depth=None, chunk=16, device=0, gains=None, **opts):
    """PhotoMap over all images, read `chunk` at a time: images is an array [M, height, width, 3] or a callable k -> [height,
    width, 3].  gains: None, or the exposure gains int64 [M, 3, 2] of all images.  Returns finish()'s dict, with the options under
    "options"."""
    R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
    M = len(R)
    with PhotoMap(points, M, intr, width, height, depth=depth, device=device, **opts) as pm:
        for k0 in range(0, M, max(int(chunk), 1)):
            k1 = min(M, k0 + max(int(chunk), 1))
            bgr = np.stack([np.asarray(images(k), np.uint8) for k in range(k0, k1)]) if callable(images) else images[k0:k1]
            pm.add_images(k0, R[k0:k1], t[k0:k1], bgr, **({} if gains is None else dict(gains=np.asarray(gains, np.int64)[k0:k1])))
        out = pm.finish()
        out["options"] = dict(pm.options)
    return out
