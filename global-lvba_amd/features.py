"""SIFT key points and descriptors of a batch of images on the GPU (lvba_sift_*; the rule is in include/lvba_hip.h).
The descriptors are what match.Matcher takes: uint8 [n, 128], a unit vector times 512.  Opt-in: importing the module loads
nothing and launches nothing; the library is looked up at the first call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.SiftOpts)


def sift_opts(lib=None, **kw):
    """lvba_sift_opts: the defaults (SiftGPU's -fo -1 -w 3 -t 0.01 -e 12; 3 intervals, sigma0 1.6, 2 orientations, 8192 features)
    with `kw` over them."""
    return L.make_opts(L.SiftOpts, "feature", **kw)


def tile_width():
    """The pixels of a row that one workgroup of the blur kernels covers."""
    return int(L.load().lvba_sift_tile_width())


def blur_taps(level, **opts):
    """float32 [2 r + 1]: the taps of the blur that makes Gaussian level `level` (0: the base blur).  Host only."""
    lib = L.load()
    taps = np.zeros(65, np.float32)
    r = C.c_int32(0)
    L.check(lib.lvba_sift_blur_taps(C.byref(sift_opts(lib, **opts)), int(level), taps.ctypes.data, C.byref(r)))
    return taps[:2 * r.value + 1].copy()


def _stack(images):
    """uint8 [n, h, w, c] (c = 1 or 3) from a sequence of equally sized [h, w] or [h, w, 3] images"""
    imgs = [np.asarray(im) for im in images]
    if not imgs:
        raise ValueError("no images")
    if any(im.dtype != np.uint8 or im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3) for im in imgs):
        raise ValueError("each image must be uint8 [h, w] (grey) or [h, w, 3] (B, G, R)")
    if any(im.shape != imgs[0].shape for im in imgs):
        raise ValueError("the images of one call must have one size and one channel count")
    a = np.ascontiguousarray(np.stack(imgs))
    return a, a.shape[2], a.shape[1], (1 if a.ndim == 3 else 3)


def octave_size(width, height, octave, first_octave=-1):
    """(w, h) of octave `octave` (first_octave, first_octave + 1, ...) of a width x height image"""
    w, h = (2 * width, 2 * height) if first_octave < 0 else (width, height)
    for _ in range(octave - first_octave):
        w, h = w // 2, h // 2
    return w, h


def extract(images, device=0, capacity=None, **opts):
    """(keypoints, descriptors, counts): per image float32 [n_i, 4] = (x, y, sigma, theta) in input pixels and uint8 [n_i, 128],
    in canonical order; counts int64 [n]: the number of features of each image before max_features cut it.  capacity: the rows the
    call may write in all (default: max_features per image); rows beyond it are missing from the last images."""
    lib = L.load()
    a, w, h, ch = _stack(images)
    o = sift_opts(lib, **opts)
    n = len(a)
    cap = int(capacity) if capacity is not None else n * max(int(o.max_features), 0)
    kp = np.zeros((cap, 4), np.float32)
    ds = np.zeros((cap, 128), np.uint8)
    off = np.zeros(n + 1, np.int64)
    counts = np.zeros(n, np.int64)
    L.check(lib.lvba_sift_extract(int(device), n, w, h, ch, a.ctypes.data, C.byref(o), cap, off.ctypes.data, kp.ctypes.data,
                                  ds.ctypes.data, counts.ctypes.data))
    lo, hi = np.minimum(off[:-1], cap), np.minimum(off[1:], cap)
    return [kp[i:j].copy() for i, j in zip(lo, hi)], [ds[i:j].copy() for i, j in zip(lo, hi)], counts


PROFILE_STAGES = ("pyramid", "detect", "orient", "describe", "host", "total")


def last_profile():
    """{stage: ms} of this thread's last extract, by the host's clock: PROFILE_STAGES."""
    ms = np.zeros(6)
    L.check(L.load().lvba_sift_profile(ms.ctypes.data))
    return dict(zip(PROFILE_STAGES, ms.tolist()))


def pyramid(image, octave, device=0, **opts):
    """(gauss float32 [S + 3, h_o, w_o], dog float32 [S + 2, h_o, w_o]) of one image's octave: a diagnostic."""
    lib = L.load()
    a, w, h, ch = _stack([image])
    o = sift_opts(lib, **opts)
    ow, oh = octave_size(w, h, int(octave), o.first_octave)
    S = max(int(o.n_intervals), 0)
    gauss = np.zeros((S + 3, max(oh, 0), max(ow, 0)), np.float32)
    dog = np.zeros((S + 2, max(oh, 0), max(ow, 0)), np.float32)
    L.check(lib.lvba_sift_pyramid(int(device), w, h, ch, a.ctypes.data, C.byref(o), int(octave), gauss.ctypes.data, dog.ctypes.data))
    return gauss, dog


def candidates(image, device=0, capacity=1 << 16, **opts):
    """(xys float32 [n, 3] = (x, y, sigma), where int32 [n, 2] = (octave, level), count): the refined key points of one image
    before the orientation, in canonical order: a diagnostic."""
    lib = L.load()
    a, w, h, ch = _stack([image])
    xys = np.zeros((int(capacity), 3), np.float32)
    where = np.zeros((int(capacity), 2), np.int32)
    count = C.c_int64(0)
    L.check(lib.lvba_sift_candidates(int(device), w, h, ch, a.ctypes.data, C.byref(sift_opts(lib, **opts)), int(capacity), xys.ctypes.data,
                                     where.ctypes.data, C.byref(count)))
    n = min(int(count.value), int(capacity))
    return xys[:n], where[:n], int(count.value)
