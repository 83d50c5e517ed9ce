"""The undistorted images of the COLMAP export (lvba_undistort_*; the rule is in include/lvba_hip.h):

    with Undistorter(intr, width, height) as und:         # the reference's defaults: same size, newK = K
        out = und.images(bgr)                             # [m, h', w', 3] uint8 from [m, height, width, 3]
        mask = und.mask()                                 # [h', w'] uint8: 255 where the pixel has a source, 0 where it is border

The poses of images.txt belong to a pinhole camera; the recorded images are Brown-Conrady ones.  Every pixel of the pinhole image
is the colour fusion's own sample of the raw image where the project's own projection puts the pixel's viewing ray, so what a
pinhole projection reads from the exported image is what the fusion read from the raw one; the exposure gains of §10r can be
applied on the way out.  Everything runs in liblvba_hip.so on the GPU; this file packs arrays.  Opt-in: nothing imports this
module unless the stage is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.UndistortOpts)


def undistort_opts(**kw):
    """lvba_undistort_opts: the defaults (the source's pinhole and size, border 0, batches of at most 64 images) with `kw` over
    them."""
    return L.make_opts(L.UndistortOpts, "undistort", **kw)


def tile():
    """(pixels per lane, tile width, tile height) of the kernel: where a test puts its sizes.  Host only."""
    v = [C.c_int32() for _ in range(3)]
    L.check(L.load().lvba_undistort_tile(*(C.byref(x) for x in v)))
    return tuple(int(x.value) for x in v)


class Undistorter(L.Handle):
    """Images of width x height through intr = fx fy cx cy k1 k2 p1 p2, to the pinhole fx fy cx cy (fx = 0: the source's) of
    out_width x out_height (0: the source's)."""
    _destroy = "lvba_undistort_free"

    def __init__(self, intr, width, height, device=0, **opts):
        self.lib = L.load()
        self.width, self.height = int(width), int(height)
        o = undistort_opts(**opts)
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_undistort_create(int(device), self.width, self.height, intr.ctypes.data, C.byref(o), C.byref(self._h)))
        w, h, nv, pin = C.c_int32(), C.c_int32(), C.c_int64(), np.zeros(4)
        L.check(self.lib.lvba_undistort_info(self._h, C.byref(w), C.byref(h), pin.ctypes.data, C.byref(nv)))
        self.size = (int(w.value), int(h.value))          # (w', h')
        self.pinhole = tuple(float(v) for v in pin)       # fx' fy' cx' cy' as resolved
        self.n_valid = int(nv.value)
        self.options = {k: getattr(o, k) for k in OPTION_NAMES}

    def images(self, bgr, gains=None):
        """bgr [m, height, width, 3] uint8 -> [m, h', w', 3] uint8.  gains: None, or the exposure gains int64 [m, 3, 2] of these
        images (expo.estimate_exposure), applied to every sample."""
        img = np.ascontiguousarray(bgr, np.uint8)
        if img.ndim != 4 or img.shape[1:] != (self.height, self.width, 3):
            raise ValueError(f"bgr {img.shape} (want [m, {self.height}, {self.width}, 3])")
        m = len(img)
        g = None if gains is None else np.ascontiguousarray(gains, np.int64)
        if g is not None and g.shape != (m, 3, 2):
            raise ValueError(f"gains {g.shape} (want [{m}, 3, 2])")
        out = np.zeros((m, self.size[1], self.size[0], 3), np.uint8)
        L.check(self.lib.lvba_undistort_images(self._h, m, img.ctypes.data, None if g is None else g.ctypes.data, out.ctypes.data))
        return out

    def map(self):
        """float64 [h', w', 2]: where each target pixel is sampled in the source, (u, v); NaN where it is not"""
        uv = np.zeros((self.size[1], self.size[0], 2))
        L.check(self.lib.lvba_undistort_map(self._h, uv.ctypes.data, None))
        return uv

    def mask(self):
        """uint8 [h', w']: 255 where the pixel is valid, 0 where it is border"""
        m = np.zeros((self.size[1], self.size[0]), np.uint8)
        L.check(self.lib.lvba_undistort_map(self._h, None, m.ctypes.data))
        return m

    def profile(self):
        """device ms of the uploads, the kernel and the downloads, accumulated over this handle's calls"""
        ms = np.zeros(3)
        L.check(self.lib.lvba_undistort_profile(self._h, ms.ctypes.data))
        return dict(upload=float(ms[0]), kernel=float(ms[1]), download=float(ms[2]))


def undistort_images(images, intr, width, height, gains=None, chunk=16, device=0, n=None, report=None, **opts):
    """Yields (k, bgr [h', w', 3]) for every image, read `chunk` at a time: images is an array [M, height, width, 3], or a
    callable k -> [height, width, 3] with n = M.  gains: None, or int64 [M, 3, 2].  report: a dict that takes size, pinhole,
    n_valid, mask, options and -- when the generator is exhausted -- profile."""
    M = int(n) if callable(images) else len(images)
    step = max(int(chunk), 1)
    g = None if gains is None else np.asarray(gains, np.int64)
    with Undistorter(intr, width, height, device=device, **opts) as und:
        if report is not None:
            report.update(size=und.size, pinhole=und.pinhole, n_valid=und.n_valid, mask=und.mask(), options=dict(und.options))
        for k0 in range(0, M, step):
            k1 = min(M, k0 + step)
            bgr = np.stack([np.asarray(images(k), np.uint8) for k in range(k0, k1)]) if callable(images) else images[k0:k1]
            out = und.images(bgr, gains=None if g is None else g[k0:k1])
            for k in range(k0, k1):
                yield k, out[k - k0]
        if report is not None:
            report["profile"] = und.profile()
