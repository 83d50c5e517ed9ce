"""Fixture of the exposure-compensation tests (tests/test_expo_host.py on the CPU, tests/test_gpu_expo.py on the GPU): the room of
photo_cases.scene(size), both sizes, all 21 images and 4 200 points, with a per-image, per-channel affine exposure planted on the
rendered colours BEFORE the rounding to a byte, then clipped to 0 .. 255.  Gains in [0.8, 1.25] and offsets in [-12, 12] grey
levels on colours in [27.5, 227.5]: the brightest tenth of an image with a high gain clips at 255 -- the saturation test is
exercised -- and most texels do not.  Seeded; nothing is committed.

The only floating-point decisions are the fusion's -- where a point is located --, and they do not depend on the colours:
photo_cases.check_margins covers them.  Everything else is integer arithmetic, so the GPU tests compare bytes."""
import functools

import numpy as np

import covis_cases as cc
import covis_oracle as co
import expo_oracle as eo
import photo_cases as pc

GAIN_RANGE = (0.8, 1.25)
OFFSET_RANGE = (-12.0, 12.0)
# the option sets the GPU tests run; `depth` is the fixture's switch (False: no depth set), the rest are lvba_expo_opts
MIN_SAMPLES = 30      # an image of the fixture sees 60 .. 470 of the 4 200 points: under the default of 200 half the images are TOO_FEW
BASE = dict(min_samples=MIN_SAMPLES)
OPTION_SETS = (BASE, dict(BASE, gate=0), dict(BASE, model=1), dict(BASE, model=1, gate=0), dict(BASE, depth=False),
               dict(BASE, depth=False, gate=0, model=1), dict())
CHUNK = 4096                                                          # csrc/expo_device.h EXPO_CHUNK
POINT_COUNTS = (0, 1, 63, 64, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, cc.N_PLANTED)


def planted_exposure(seed=23):
    """(gain [21, 3], offset [21, 3] in grey levels): log-uniform gains, uniform offsets, per image and channel (b, g, r)"""
    rng = np.random.default_rng(seed)
    gain = np.exp(rng.uniform(np.log(GAIN_RANGE[0]), np.log(GAIN_RANGE[1]), (cc.N_IMAGES, 3)))
    offset = rng.uniform(OFFSET_RANGE[0], OFFSET_RANGE[1], (cc.N_IMAGES, 3))
    return gain, offset


def render_float(intr, Rcw, C, W, H):
    """float64 [H, W, 3]: the planted colour of the wall point along the undistorted ray of every pixel, before any rounding"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y, ok = co.undistort(intr, u.ravel(), v.ravel())
    assert ok.all()
    dirs = np.stack([x, y, np.ones_like(x)], 1) @ Rcw
    s = cc.cast(C, dirs)
    return pc.planted_colour(C + s[:, None] * dirs).reshape(H, W, 3)


@functools.lru_cache(None)
def scene(size=0):
    """photo_cases.scene(size) with `images` the exposed ones, `clean` the unexposed ones, and the planted `gain`, `offset`"""
    r = dict(pc.scene(size))
    gain, offset = planted_exposure()
    r["clean"] = r["images"]
    exposed = []
    for k in range(cc.N_IMAGES):
        f = render_float(r["intr"], r["Rcw"][k], r["C"][k], r["W"], r["H"])
        assert (np.floor(f + 0.5).astype(np.uint8) == r["clean"][k]).all()       # the same render as photo_cases'
        exposed.append(np.clip(np.floor(gain[k] * f + offset[k] + 0.5), 0, 255).astype(np.uint8))
    r["images"] = np.ascontiguousarray(np.stack(exposed))
    r["gain"], r["offset"] = gain, offset
    return r


def split(kw):
    """an option set -> (use the depth set, the library's options)"""
    kw = dict(kw)
    return kw.pop("depth", True), kw


@functools.lru_cache(None)
def _estimate(size, key, rounds, exposed):
    s = scene(size)
    with_depth, opts = split(dict(key))
    return eo.estimate(s["points"], s["images"] if exposed else s["clean"], s["depth"] if with_depth else None, s["intr"], s["Rcw"], s["tcw"],
                       rounds=rounds, **opts)


def estimate(size, rounds=3, exposed=True, **kw):
    """the oracle's alternation on all points and all 21 images under an option set (computed once; do not write into it)"""
    return _estimate(size, pc.key_of(kw), rounds, exposed)


@functools.lru_cache(None)
def _first_round(size, key):
    """(ref16, valid, gains_in, sums) of a round of the alternation that has gains to apply: the reference of the fusion under the
    first round's gains, and the oracle's sums under them"""
    s = scene(size)
    with_depth, opts = split(dict(key))
    depth = s["depth"] if with_depth else None
    gains = estimate(size, rounds=1, **dict(key))["gains"]
    nv, S1, _ = eo.fuse(s["points"], s["images"], depth, s["intr"], s["Rcw"], s["tcw"], gains, **opts)
    ref16, valid = eo.reference(nv, S1)
    return ref16, valid, gains, eo.sums(s["points"], s["images"], depth, s["intr"], s["Rcw"], s["tcw"], ref16, valid, gains, **opts)


def second_round(size, **kw):
    """what the second round of the alternation hands the sums pass, and what it must return (computed once)"""
    return _first_round(size, pc.key_of(kw))


def planted_inverse(status):
    """float64 [21, 3, 2]: the gains that undo the planted exposure, (1 / gain, -offset / gain in grey levels), brought to the gauge
    of the solve over the images that are OK or FALLBACK_GAIN: mean gain 1, mean offset 0"""
    gain, offset = planted_exposure()
    A, B = 1.0 / gain, -offset / gain
    ok = np.asarray(status) <= eo.FALLBACK_GAIN
    S = 1.0 / A[ok].mean(0)
    A, B = A * S, B * S
    return np.stack([A, B - B[ok].mean(0)], -1)


def constant_case(size, seed=5):
    """The closed form: image j one colour v_j (per channel, 60 .. 235: unsaturated), the reference one colour r: D = 0, every
    channel falls back to the gain-only form and A_j = (256 r 2^16 + 256 v_j / 2) // (256 v_j) before the gauge.  dict(images,
    colours int64 [21, 3], ref int64 [3], ref16 uint16 [n, 3], valid uint8 [n])"""
    s = scene(size)
    rng = np.random.default_rng(seed)
    colours = rng.integers(60, 236, (cc.N_IMAGES, 3)).astype(np.int64)        # r / v in [0.42, 2.5]: inside the gain bounds
    ref = np.array([100, 128, 150], np.int64)
    img = np.ascontiguousarray(np.broadcast_to(colours[:, None, None, :].astype(np.uint8), (cc.N_IMAGES, s["H"], s["W"], 3)))
    n = len(s["points"])
    return dict(images=img, colours=colours, ref=ref, ref16=np.ascontiguousarray(np.broadcast_to((256 * ref).astype(np.uint16), (n, 3))),
                valid=np.ones(n, np.uint8))
