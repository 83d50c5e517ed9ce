"""Per-image exposure compensation of the colour fusion (lvba_expo_*; the rule is in include/lvba_hip.h):

    rep = estimate_exposure(points, images, Rcw, tcw, intr, width, height, depth=depth_images)   # gains int64 [M, 3, 2], report
    photo.photo_consistency(points, images, Rcw, tcw, intr, width, height, depth=depth_images, gains=rep["gains"])

A camera with auto-exposure sees one wall brighter in some frames than in others; the fusion's spread then measures exposure, not
geometry.  A gain and an offset per image and channel are estimated against the fused colours and the fusion applies them, the
two in alternation.  The sums run in liblvba_hip.so on the GPU, the solve is the library's integer arithmetic on the host; this
file packs arrays.  Opt-in: nothing imports this module unless the stage is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.ExpoOpts)
STATUS = {0: "OK", 1: "FALLBACK_GAIN", 2: "TOO_FEW_SAMPLES", 3: "OUT_OF_BOUNDS"}
OK, FALLBACK_GAIN, TOO_FEW_SAMPLES, OUT_OF_BOUNDS = range(4)
AFFINE, GAIN = 0, 1
N_SUMS = 20
ONE = 65536


def expo_opts(**kw):
    """lvba_expo_opts: the defaults (the fusion's occlusion test, the affine model, texel bytes in 4 .. 251, a gate of 30 grey
    levels, 200 samples, 2 grey levels of spread, gains in 0.25 .. 4, offsets up to 64 grey levels; all of them this library's
    choice, none tuned on recorded data) with `kw` over them."""
    return L.make_opts(L.ExpoOpts, "exposure compensation", **kw)


def identity_gains(m):
    """int64 [m, 3, 2]: (65536, 0) throughout"""
    g = np.zeros((int(m), 3, 2), np.int64)
    g[:, :, 0] = ONE
    return g


def gains_float(gains):
    """float64 [m, 3, 2]: A / 65536 and B / (65536 * 256), the offset in grey levels"""
    g = np.asarray(gains, np.int64).astype(np.float64)
    return np.stack([g[..., 0] / ONE, g[..., 1] / (ONE * 256.0)], -1)


def solve_gains(sums, **opts):
    """lvba_expo_solve on sums uint64 [m, 20]: (gains int64 [m, 3, 2], status int32 [m]).  Host arithmetic only, no device."""
    s = np.ascontiguousarray(sums, np.uint64).reshape(-1, N_SUMS)
    o = expo_opts(**opts)
    gains, status = identity_gains(len(s)), np.zeros(len(s), np.int32)
    L.check(L.load().lvba_expo_solve(len(s), s.ctypes.data, C.byref(o), gains.ctypes.data, status.ctypes.data))
    return gains, status


class ExposureEstimator(L.Handle):
    """`points` [n, 3] (float32 world points) with their reference colours ref16 [n, 3] (uint16; b, g, r in 1/256 grey level) and
    validity bytes valid [n] (palign.reference_from_sums), against n_images images of width x height through intr = fx fy cx cy k1
    k2 p1 p2.  depth: a visual.DepthImages of the same images (the occlusion test), kept alive by the caller, or None."""
    _destroy = "lvba_expo_free"

    def __init__(self, points, ref16, valid, n_images, width, height, intr, depth=None, device=0, **opts):
        self.lib = L.load()
        xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(ref16, np.uint16).reshape(-1, 3)
        ok = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if len(ref) != len(xyz) or len(ok) != len(xyz):
            raise ValueError(f"{len(xyz)} points, {len(ref)} reference colours, {len(ok)} validity bytes")
        self.n, self.n_images, self.width, self.height = len(xyz), int(n_images), int(width), int(height)
        self.depth = depth
        o = expo_opts(**opts)
        self.options = {k: getattr(o, k) for k in OPTION_NAMES}
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_expo_create(int(device), self.n, xyz.ctypes.data, ref.ctypes.data, ok.ctypes.data, self.n_images, self.width,
                                          self.height, intr.ctypes.data, depth._h if depth is not None else None, C.byref(o),
                                          C.byref(self._h)))

    def sums(self, first, Rcw, tcw, bgr, gains=None):
        """The 20 estimation sums of images first .. first + m - 1 under `gains` (int64 [m, 3, 2]; None: identity): uint64 [m, 20]."""
        R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9)
        t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
        img = np.ascontiguousarray(bgr, np.uint8)
        m = len(R)
        if len(t) != m or img.shape != (m, self.height, self.width, 3):
            raise ValueError(f"{m} rotations, {len(t)} translations, bgr {img.shape} (want [{m}, {self.height}, {self.width}, 3])")
        g = None if gains is None else np.ascontiguousarray(gains, np.int64)
        if g is not None and g.shape != (m, 3, 2):
            raise ValueError(f"gains {g.shape} (want [{m}, 3, 2])")
        out = np.zeros((m, N_SUMS), np.uint64)
        L.check(self.lib.lvba_expo_sums(self._h, int(first), m, R.ctypes.data, t.ctypes.data, img.ctypes.data,
                                        None if g is None else g.ctypes.data, out.ctypes.data))
        return out

    def profile(self):
        """device ms of the uploads and the sums passes, accumulated over this handle's calls"""
        ms = np.zeros(2)
        L.check(self.lib.lvba_expo_profile(self._h, ms.ctypes.data))
        return dict(upload=float(ms[0]), sums=float(ms[1]))


def rmse_of_sums(sums):
    """float64 [m]: sqrt(sum (c' - ref)^2 / n) / 256 over an image's three channels, in grey levels; 0 without a used term"""
    s = np.asarray(sums, np.uint64).reshape(-1, N_SUMS)
    n = s[:, 0:18:6].astype(np.float64).sum(1)
    e = s[:, 5:18:6].astype(np.float64).sum(1)
    return np.where(n > 0, np.sqrt(e / np.maximum(n, 1.0)) / 256.0, 0.0)


def estimate_exposure(points, images, Rcw, tcw, intr, width, height, depth=None, rounds=3, min_views=2, chunk=16, device=0, **opts):
    """The alternation, as pipeline.align_cameras_photometric drives its own.  images: an array [M, H, W, 3] or a callable k ->
    [H, W, 3], read `chunk` at a time.  Per round: (1) the colour fusion with the current gains gives the integer sums and the
    spread; (2) the reference colours are the fused ones (palign.reference_from_sums), points below min_views invalid; (3) the 20
    sums of every image against them, gate and residual under the current gains; (4) the solve and the gauge give the next gains.
    Returns dict(gains int64 [M, 3, 2], gains_float, status [M], status_names, mean_sigma [rounds + 1]: the spread from before any
    compensation to the final one, rounds: per round dict(mean_sigma, rmse [M], n_used [M], max_gain_change, status), sums: the
    last round's, options).  rounds = 3 is a default, not a convergence claim: the alternation is block-coordinate descent, and
    along a corridor a correction travels one overlap per round.  opts: expo_opts' options."""
    from .palign import reference_from_sums
    from .photo import PhotoMap
    R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 3, 3)
    t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
    M, step = len(R), max(int(chunk), 1)
    read = (lambda a, b: np.stack([np.asarray(images(k), np.uint8) for k in range(a, b)])) if callable(images) else (lambda a, b: images[a:b])
    occl = {k: opts[k] for k in ("occlusion_rel", "occlusion_abs", "max_depth", "holes") if k in opts}
    spans = [(k0, min(M, k0 + step)) for k0 in range(0, M, step)]

    def fuse(gains):
        """the fusion under `gains`: (mean spread, (n_views, s1, s2))"""
        with PhotoMap(points, M, intr, width, height, depth=depth, device=device, min_views=max(int(min_views), 2), **occl) as pm:
            for k0, k1 in spans:
                pm.add_images(k0, R[k0:k1], t[k0:k1], read(k0, k1), gains=gains[k0:k1])
            return pm.finish()["summary"]["mean_sigma"], pm.sums()

    gains = identity_gains(M)
    status = np.zeros(M, np.int32)
    out = dict(mean_sigma=[], rounds=[])
    sums = np.zeros((M, N_SUMS), np.uint64)
    for _ in range(max(int(rounds), 1)):
        spread, fused = fuse(gains)
        out["mean_sigma"].append(spread)
        ref16, valid = reference_from_sums(fused[0], fused[1], min_views)
        with ExposureEstimator(points, ref16, valid, M, width, height, intr, depth=depth, device=device, **opts) as est:
            sums = np.concatenate([est.sums(k0, R[k0:k1], t[k0:k1], read(k0, k1), gains=gains[k0:k1]) for k0, k1 in spans])
            out["options"] = dict(est.options)
        new, status = solve_gains(sums, **opts)
        change = float(np.abs(new[:, :, 0] - gains[:, :, 0]).max(initial=0)) / ONE
        out["rounds"].append(dict(mean_sigma=spread, rmse=rmse_of_sums(sums), n_used=sums[:, 0:18:6].sum(1).astype(np.int64),
                                  max_gain_change=change, status=status.copy()))
        gains = new
    out["mean_sigma"].append(fuse(gains)[0])
    out.update(gains=gains, gains_float=gains_float(gains), status=status, status_names=[STATUS[int(v)] for v in status], sums=sums)
    return out
