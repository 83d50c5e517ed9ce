"""GPU tests of the per-image exposure compensation (lvba_expo_*, lvba_photo_add_images_gains; csrc/expo.hip, csrc/photo.hip;
DESIGN.md §10r) against the integer restatement (tests/expo_oracle.py) on the exposed room of tests/expo_cases.py.  Sums, gains,
statuses, rgb and sigma compare exactly: where a point is located is covered by the fixture's margin condition
(photo_cases.check_margins, asserted on the CPU), and everything after that is integer arithmetic."""
import ctypes
import importlib
import json
import math

import numpy as np
import pytest

import covis_cases as cc
import expo_cases as ec
import expo_oracle as eo
import photo_cases as pc
import photo_oracle as po

pytestmark = pytest.mark.gpu


def _mods():
    return (importlib.import_module("global-lvba_amd"), importlib.import_module("global-lvba_amd.expo"),
            importlib.import_module("global-lvba_amd.photo"), importlib.import_module("global-lvba_amd.visual"),
            importlib.import_module("global-lvba_amd.pipeline"))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_sums(points, images, depth, intr, Rcw, tcw, ref16, valid, gains=None, calls=None, **opts):
    """uint64 [M, 20] by image index: the images brought by calls [(first, count), ...] (default: one call)"""
    _, EX, _, V, _ = _mods()
    M, W, H = len(images), images.shape[2], images.shape[1]
    dset = V.DepthImages.upload(depth) if depth is not None else None
    out = np.zeros((M, eo.N_SUMS), np.uint64)
    try:
        with EX.ExposureEstimator(points, ref16, valid, M, W, H, intr, depth=dset, **opts) as est:
            for a, m in (calls if calls is not None else [(0, M)]):
                out[a:a + m] = est.sums(a, Rcw[a:a + m], tcw[a:a + m], images[a:a + m], gains=None if gains is None else gains[a:a + m])
            prof = est.profile()
            assert prof["upload"] >= 0 and prof["sums"] >= 0
    finally:
        if dset is not None:
            dset.close()
    return out


def run_fuse(points, images, depth, intr, Rcw, tcw, gains="plain", calls=None, **opts):
    """the fusion: dict(sums, n_views, rgb, sigma, summary); gains "plain": lvba_photo_add_images, else the gains entry point"""
    _, _, PH, V, _ = _mods()
    M, W, H = len(images), images.shape[2], images.shape[1]
    dset = V.DepthImages.upload(depth) if depth is not None else None
    try:
        with PH.PhotoMap(points, M, intr, W, H, depth=dset, **opts) as pm:
            for a, m in (calls if calls is not None else [(0, M)]):
                if isinstance(gains, str) and gains == "null":                                            # the gains entry point with gains == NULL
                    R, t, img = (np.ascontiguousarray(q[a:a + m]) for q in (Rcw, tcw, images))
                    assert pm.lib.lvba_photo_add_images_gains(pm._h, a, m, R.ctypes.data, t.ctypes.data, img.ctypes.data, None) == 0
                elif isinstance(gains, str):
                    pm.add_images(a, Rcw[a:a + m], tcw[a:a + m], images[a:a + m])
                else:
                    pm.add_images(a, Rcw[a:a + m], tcw[a:a + m], images[a:a + m], gains=gains[a:a + m])
            out = pm.finish()
            out["sums"] = pm.sums()
            return out
    finally:
        if dset is not None:
            dset.close()


def scene_args(s, with_depth=True, n=None):
    return (s["points"][:n], s["images"], s["depth"] if with_depth else None, s["intr"], s["Rcw"], s["tcw"])


# ------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
@pytest.mark.parametrize("option_set", range(len(ec.OPTION_SETS)))
def test_sums_equal_the_oracle(size, option_set):
    """every image's 20 sums: both sizes, both models, gate 0 and 30, with and without a depth set; under a first round's gains and
    under none"""
    kw = ec.OPTION_SETS[option_set]
    with_depth, opts = ec.split(kw)
    ref16, valid, gains, want = ec.second_round(size, **kw)
    args = scene_args(ec.scene(size), with_depth)
    assert same_bytes(run_sums(*args, ref16, valid, gains, **opts), want), kw
    plain = eo.sums(*args, ref16, valid, None, **opts)
    assert same_bytes(run_sums(*args, ref16, valid, None, **opts), plain), kw
    assert same_bytes(run_sums(*args, ref16, valid, eo.identity(cc.N_IMAGES), **opts), plain), kw


# ------------------------------------------------------------------------------------------------------------ 2. chunk edges
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_chunk_edges(size):
    """the first 0, 1, 63, 64, 255, 256, 257, 4095, 4096, 4097 and all 4 200 points: a wavefront, a workgroup's round of 256 and the
    sums kernel's chunk of 4096"""
    s = ec.scene(size)
    ref16, valid, gains, _ = ec.second_round(size, **ec.BASE)
    _, opts = ec.split(ec.BASE)
    for n in ec.POINT_COUNTS:
        args = scene_args(s, n=n)
        got = run_sums(*args, ref16[:n], valid[:n], gains, **opts)
        assert same_bytes(got, eo.sums(*args, ref16[:n], valid[:n], gains, **opts)), n

# ---------------------------------------------------------------------------------------------------- 3. batching independence
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_same_bytes_for_any_batching(size):
    ref16, valid, gains, want = ec.second_round(size, **ec.BASE)
    _, opts = ec.split(ec.BASE)
    args = scene_args(ec.scene(size))
    M = cc.N_IMAGES
    one = [(k, 1) for k in range(M)]
    for kw in (dict(calls=one), dict(calls=one[::-1]), dict(max_batch_images=1), dict(max_batch_images=2), dict(max_batch_images=3),
               dict(calls=[(5, 16), (0, 5)], max_batch_images=3)):
        assert same_bytes(run_sums(*args, ref16, valid, gains, **dict(opts, **kw)), want), kw


# --------------------------------------------------------------------------------------------------------- 4. fusion with gains
def assert_fusion(got, nv, S1, S2, min_views=2, msg=""):
    rgb, sigma = po.finish(nv, S1, S2, min_views=min_views)
    a, b, c = got["sums"]
    assert same_bytes(a, nv) and same_bytes(b, S1) and same_bytes(c, S2), msg
    assert same_bytes(got["n_views"], nv) and same_bytes(got["rgb"], rgb) and same_bytes(got["sigma"], sigma), msg


@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_fusion_with_gains(size):
    s = ec.scene(size)
    M = cc.N_IMAGES
    for with_depth in (True, False):
        args = scene_args(s, with_depth)
        plain = run_fuse(*args)
        for g in ("null", eo.identity(M)):                                       # NULL and identity: the bytes of lvba_photo_add_images
            got = run_fuse(*args, gains=g)
            for a, b in zip(got["sums"], plain["sums"]):
                assert same_bytes(a, b)
            assert same_bytes(got["rgb"], plain["rgb"]) and same_bytes(got["sigma"], plain["sigma"])
            assert np.float64(got["summary"]["mean_sigma"]).tobytes() == np.float64(plain["summary"]["mean_sigma"]).tobytes()
        gains = ec.second_round(size, **dict(ec.BASE, depth=with_depth))[2]
        assert (gains != eo.identity(M)).any()
        want = eo.fuse(*args, gains)
        assert_fusion(run_fuse(*args, gains=gains), *want, msg="estimated gains")
        one = [(k, 1) for k in range(M)]
        assert_fusion(run_fuse(*args, gains=gains, calls=one[::-1], max_batch_images=2), *want, msg="one image per call, reversed")
    # gains that drive samples into both ends of the clamp: c' = 4 c - 255 grey levels is 0 below 63.75 and 65 280 above 127.5
    args = scene_args(s)
    both = eo.identity(M)
    both[:, :, 0], both[:, :, 1] = eo.A_MAX, -eo.B_MAX
    both[0], both[1] = [eo.A_MAX, eo.B_MAX], [eo.A_MIN, -eo.B_MAX]              # image 0 all white, image 1 all black
    nv, S1, S2 = eo.fuse(*args, both)
    single = eo.fuse(s["points"], s["images"][2:3], s["depth"][2:3], s["intr"], s["Rcw"][2:3], s["tcw"][2:3], both[2:3])
    seen = single[0] > 0
    assert (single[1][seen] == 0).any() and (single[1][seen] == eo.C_MAX).any() and ((single[1][seen] > 0) & (single[1][seen] < eo.C_MAX)).any()
    assert_fusion(run_fuse(*args, gains=both), nv, S1, S2, msg="both ends of the clamp")


# -------------------------------------------------------------------------------------------------------- 5. the closed form
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_constant_colour_closed_form(size):
    """image j one colour v_j, the reference one colour r: the sums follow from how many points an image sees, D = 0, every image
    with samples is FALLBACK_GAIN with A_j = (r 2^16 + v_j / 2) // v_j before the gauge"""
    _, EX, _, _, _ = _mods()
    s = ec.scene(size)
    c = ec.constant_case(size)
    sums = run_sums(s["points"], c["images"], s["depth"], s["intr"], s["Rcw"], s["tcw"], c["ref16"], c["valid"], gate=0)
    seen = pc.expected(size)["seen"].sum(1)
    v, r = 256 * c["colours"], 256 * c["ref"]
    for j in range(cc.N_IMAGES):
        n = int(seen[j])
        for k in range(3):
            vv, rr = int(v[j, k]), int(r[k])
            assert sums[j, 6 * k:6 * k + 6].tolist() == [n, n * vv, n * rr, n * vv * vv, n * vv * rr, n * (vv - rr) ** 2], (j, k)
        assert sums[j, 18] == n and sums[j, 19] == 0
    gains, status = EX.solve_gains(sums, min_samples=ec.MIN_SAMPLES)
    live = seen >= ec.MIN_SAMPLES
    assert (status[live] == EX.FALLBACK_GAIN).all() and (status[~live] == EX.TOO_FEW_SAMPLES).all()
    for k in range(3):
        A = [(int(r[k]) * 65536 + int(v[j, k]) // 2) // int(v[j, k]) for j in np.flatnonzero(live)]
        S = (len(A) * 2 ** 32 + sum(A) // 2) // sum(A)
        assert gains[live, k, 0].tolist() == [(a * S + 32768) >> 16 for a in A] and not gains[live, k, 1].any()


# ------------------------------------------------------------------------------------------------- 6. the solve, the alternation
def test_solve_gives_the_oracles_bytes():
    _, EX, _, _, _ = _mods()
    for size in range(len(cc.SIZES)):
        for kw in ec.OPTION_SETS:
            _, opts = ec.split(kw)
            sums = ec.second_round(size, **kw)[3]
            gains, status = EX.solve_gains(sums, **opts)
            want_g, want_s = eo.solve(sums, **opts)
            assert same_bytes(gains, want_g) and same_bytes(status, want_s), (size, kw)


@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_estimate_exposure_end_to_end(size):
    """the alternation through the library equals the oracle's: gains and statuses as bytes, every round's sums-derived figures, and
    the spreads within the summation bound of the fusion's summary ((n_valid + 1) 2^-53 relative: non-negative terms)"""
    _, EX, _, V, _ = _mods()
    s = ec.scene(size)
    for kw in (ec.BASE, dict(ec.BASE, model=1, gate=0)):
        _, opts = ec.split(kw)
        e = ec.estimate(size, **kw)
        with V.DepthImages.upload(s["depth"]) as depth:
            got = EX.estimate_exposure(s["points"], lambda k: s["images"][k], s["Rcw"], s["tcw"], s["intr"], s["W"], s["H"], depth=depth, chunk=5,
                                       **opts)
        assert same_bytes(got["gains"], e["gains"]) and same_bytes(got["status"], e["status"]) and same_bytes(got["sums"], e["sums"]), kw
        assert got["status_names"] == [EX.STATUS[int(v)] for v in e["status"]] and len(got["mean_sigma"]) == 4 == len(e["mean_sigma"])
        assert same_bytes(got["gains_float"], EX.gains_float(e["gains"])) and got["gains_float"][e["status"] >= 2].tolist() == [[[1.0, 0.0]] * 3] * int((e["status"] >= 2).sum())
        n_valid = len(s["points"])
        for a, b in zip(got["mean_sigma"], e["mean_sigma"]):
            assert abs(a - b) <= (n_valid + 1) * 2.0 ** -53 * b, kw
        for a, b in zip(got["rounds"], e["rounds"]):
            assert same_bytes(a["rmse"], b["rmse"]) and a["max_gain_change"] == b["max_gain_change"] and same_bytes(a["status"], b["status"])
        assert got["options"]["min_samples"] == ec.MIN_SAMPLES
        print(f"size {cc.SIZES[size]} {kw}: spread per round {got['mean_sigma']}")


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_invalid_arguments_are_refused():
    """every refusal of the header's list: LVBA_ERR_ARG, nothing written, the handle usable afterwards"""
    pkg, EX, PH, V, _ = _mods()
    L = pkg._lib
    lib = ctypes.CDLL(L.LIB_PATH)                           # raw prototypes: NULL pointers go through as they are
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.lvba_expo_create.argtypes = [i32, i64, vp, vp, vp, i32, i32, i32, vp, vp, vp, ctypes.POINTER(vp)]
    lib.lvba_expo_sums.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.lvba_expo_solve.argtypes = [i32, vp, vp, vp, vp]
    lib.lvba_expo_profile.argtypes = [vp, vp]
    lib.lvba_expo_free.argtypes = [vp]
    lib.lvba_expo_free.restype = None
    lib.lvba_photo_create.argtypes = [i32, i64, vp, i32, i32, i32, vp, vp, vp, ctypes.POINTER(vp)]
    lib.lvba_photo_add_images_gains.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.lvba_photo_sums.argtypes = [vp, vp, vp, vp]
    lib.lvba_photo_free.argtypes = [vp]
    lib.lvba_photo_free.restype = None
    lib.lvba_last_error.restype = ctypes.c_char_p
    s = ec.scene(1)
    W, H, M = s["W"], s["H"], cc.N_IMAGES
    ptr = lambda a: a.ctypes.data
    pts, intr = s["points"], np.ascontiguousarray(s["intr"])
    n = len(pts)
    ref16, valid, gains, want = ec.second_round(1, **ec.BASE)
    ref16, valid, gains = np.ascontiguousarray(ref16), np.ascontiguousarray(valid), np.ascontiguousarray(gains)
    SENTINEL = 0x5A5A
    h = vp(SENTINEL)

    def create(dev=0, n=n, P=pts, Rf=ref16, Vd=valid, M=M, w=W, hh=H, I=intr, depth=None, out=True, **o):
        h.value = SENTINEL
        opts = EX.expo_opts() if o else None
        for k, v in o.items():
            setattr(opts, k, v)                                                  # past make_opts' coercion: NaN, negatives
        return lib.lvba_expo_create(dev, n, ptr(P) if P is not None else None, ptr(Rf) if Rf is not None else None,
                                    ptr(Vd) if Vd is not None else None, M, w, hh, ptr(I) if I is not None else None, depth,
                                    ctypes.byref(opts) if opts is not None else None, ctypes.byref(h) if out else None)

    def refused(rc):
        return rc == L.ERR_ARG and h.value == SENTINEL                           # nothing written

    assert refused(create(P=None)) and refused(create(Rf=None)) and refused(create(Vd=None)) and refused(create(I=None))
    assert create(out=False) == L.ERR_ARG
    assert refused(create(n=-1)) and refused(create(n=2 ** 32))
    assert refused(create(w=1)) and refused(create(hh=1))
    assert refused(create(M=0)) and refused(create(M=32769))
    for k in range(8):
        bad = intr.copy(); bad[k] = np.nan
        assert refused(create(I=bad)), k
    for k in (0, 1):
        bad = intr.copy(); bad[k] = 0.0
        assert refused(create(I=bad)) and b"focal" in lib.lvba_last_error()
    for name in ("occlusion_rel", "occlusion_abs", "max_depth"):
        for v in (-1e-3, np.nan, np.inf):
            assert refused(create(**{name: v})), (name, v)
    BAD_OPTS = (dict(max_batch_images=-1), dict(model=2), dict(model=-1), dict(sat_lo=-1), dict(sat_hi=256), dict(sat_lo=9, sat_hi=8), dict(gate=-1),
                dict(gate=256), dict(min_samples=1), dict(min_spread=-1), dict(min_spread=256), dict(min_gain=0.2), dict(min_gain=1.5),
                dict(max_gain=0.9), dict(max_gain=4.5), dict(max_offset=-1.0), dict(max_offset=256.0), dict(min_gain=np.nan), dict(max_gain=np.nan),
                dict(max_offset=np.nan))
    for o in BAD_OPTS:
        assert refused(create(**o)), o
    high = ref16.copy(); high[17, 1] = 65281
    assert refused(create(Rf=high)) and b"reference" in lib.lvba_last_error()
    with V.DepthImages.upload(s["depth"][:5]) as few, V.DepthImages.upload(ec.scene(0)["depth"]) as other_size:
        assert refused(create(depth=few._h)) and refused(create(depth=other_size._h))
        assert b"depth set" in lib.lvba_last_error()
    R, t, img = np.ascontiguousarray(s["Rcw"]), np.ascontiguousarray(s["tcw"]), s["images"]
    FILL = np.uint64(0x7777)
    out = np.full((M, eo.N_SUMS), FILL, np.uint64)
    with V.DepthImages.upload(s["depth"]) as depth:
        assert create(depth=depth._h, min_samples=ec.MIN_SAMPLES) == L.OK and h.value not in (None, SENTINEL)
        sums = lambda first, m, R=R, t=t, img=img, g=gains, o=out, hh=h: lib.lvba_expo_sums(
            hh, first, m, ptr(R[first:]) if R is not None else None, ptr(t[first:]) if t is not None else None,
            ptr(img[first:]) if img is not None else None, ptr(g[first:]) if g is not None else None, ptr(o[first:]) if o is not None else None)
        untouched = lambda: (out == FILL).all()
        assert sums(0, 1, hh=None) == L.ERR_ARG
        assert sums(-1, 2) == L.ERR_ARG and sums(0, -1) == L.ERR_ARG and sums(M, 1) == L.ERR_ARG and sums(M - 1, 2) == L.ERR_ARG
        assert sums(0, 2, R=None) == L.ERR_ARG and sums(0, 2, t=None) == L.ERR_ARG and sums(0, 2, img=None) == L.ERR_ARG
        assert sums(0, 2, o=None) == L.ERR_ARG
        badR = R.copy(); badR[1, 0, 0] = np.nan
        assert sums(0, 2, R=badR) == L.ERR_ARG and b"camera 1: non-finite rotation" in lib.lvba_last_error()
        badt = t.copy(); badt[0, 2] = np.inf
        assert sums(0, 2, t=badt) == L.ERR_ARG and b"non-finite translation" in lib.lvba_last_error()
        for where, v in (((1, 0, 0), eo.A_MIN - 1), ((1, 2, 0), eo.A_MAX + 1), ((0, 1, 1), eo.B_MAX + 1), ((1, 1, 1), -eo.B_MAX - 1)):
            badg = gains.copy(); badg[where] = v
            assert sums(0, 2, g=badg) == L.ERR_ARG and b"gains" in lib.lvba_last_error(), where
        assert untouched()
        assert sums(0, 0) == L.OK and untouched()                                # no image: nothing to write
        assert sums(0, M) == L.OK and same_bytes(out, want)                      # still usable, and the right bytes
        assert sums(3, 4, g=None) == L.OK                                        # gains_in may be NULL
        ms = np.full(2, -1.0)
        assert lib.lvba_expo_profile(None, ptr(ms)) == L.ERR_ARG and lib.lvba_expo_profile(h, None) == L.ERR_ARG and (ms == -1.0).all()
        assert lib.lvba_expo_profile(h, ptr(ms)) == L.OK and (ms >= 0).all() and ms[1] > 0
        lib.lvba_expo_free(h)
        lib.lvba_expo_free(None)
        # the fusion's gains entry point
        hp = vp()
        assert lib.lvba_photo_create(0, n, ptr(pts), M, W, H, ptr(intr), depth._h, None, ctypes.byref(hp)) == L.OK
        add = lambda first, m, R=R, t=t, img=img, g=gains, hh=hp: lib.lvba_photo_add_images_gains(
            hh, first, m, ptr(R[first:]) if R is not None else None, ptr(t[first:]) if t is not None else None,
            ptr(img[first:]) if img is not None else None, ptr(g[first:]) if g is not None else None)
        assert add(0, 1, hh=None) == L.ERR_ARG and add(-1, 2) == L.ERR_ARG and add(M - 1, 2) == L.ERR_ARG and add(0, -1) == L.ERR_ARG
        assert add(0, 2, R=None) == L.ERR_ARG and add(0, 2, t=None) == L.ERR_ARG and add(0, 2, img=None) == L.ERR_ARG
        assert add(0, 2, R=badR) == L.ERR_ARG and add(0, 2, t=badt) == L.ERR_ARG
        for where, v in (((1, 0, 0), eo.A_MIN - 1), ((1, 2, 0), eo.A_MAX + 1), ((0, 1, 1), eo.B_MAX + 1), ((1, 1, 1), -eo.B_MAX - 1)):
            badg = gains.copy(); badg[where] = v
            assert add(0, 2, g=badg) == L.ERR_ARG and b"gains" in lib.lvba_last_error(), where
        nv = np.full(n, 7, np.int32)
        assert lib.lvba_photo_sums(hp, ptr(nv), None, None) == L.OK and not nv.any()               # the refusals added nothing
        assert add(3, 4) == L.OK and add(6, 2) == L.ERR_ARG and b"added before" in lib.lvba_last_error()
        assert add(0, 3) == L.OK and add(7, M - 7) == L.OK                                         # still usable
        s1, s2 = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.int64)
        assert lib.lvba_photo_sums(hp, ptr(nv), ptr(s1), ptr(s2)) == L.OK
        wv, w1, w2 = eo.fuse(pts, img, s["depth"], intr, R, t, gains)
        assert same_bytes(nv, wv) and same_bytes(s1, w1) and same_bytes(s2, w2)
        lib.lvba_photo_free(hp)
    # the solve: no device
    g_out, st_out = np.full((M, 3, 2), 7, np.int64), np.full(M, 7, np.int32)
    solve = lambda m=M, S=want, o=None, G=g_out, St=st_out: lib.lvba_expo_solve(m, ptr(S) if S is not None else None, ctypes.byref(o) if o is not None else None,
                                                                              ptr(G) if G is not None else None, ptr(St) if St is not None else None)
    clean = lambda: (g_out == 7).all() and (st_out == 7).all()
    assert solve(m=-1) == L.ERR_ARG and solve(m=32769) == L.ERR_ARG and solve(S=None) == L.ERR_ARG and solve(G=None) == L.ERR_ARG
    assert solve(St=None) == L.ERR_ARG and clean()
    for o in BAD_OPTS[1:]:
        opts = EX.expo_opts()
        for k, v in o.items():
            setattr(opts, k, v)
        assert solve(o=opts) == L.ERR_ARG and clean(), o
    for col, v in ((0, 2 ** 32), (1, 2 ** 62), (2, 2 ** 62), (3, 2 ** 63), (10, 2 ** 63)):
        bad = want.copy(); bad[4, col] = np.uint64(v)
        assert solve(S=bad) == L.ERR_ARG and b"sums of image 4" in lib.lvba_last_error() and clean(), col
    assert solve(m=0) == L.OK and clean()
    assert solve(o=EX.expo_opts(min_samples=ec.MIN_SAMPLES)) == L.OK
    wg, ws = eo.solve(want, **ec.BASE)
    assert same_bytes(g_out, wg) and same_bytes(st_out, ws)
    assert pkg._lib.load().lvba_version() == 112
    with pytest.raises(TypeError):
        EX.ExposureEstimator(pts, ref16, valid, M, W, H, intr, no_such_option=1)
    with pytest.raises(ValueError):
        EX.ExposureEstimator(pts, ref16[:-1], valid, M, W, H, intr)


def test_non_finite_points_keep_their_index():
    """NaN and +-inf coordinates: such a point is never located, in the sums and in the fusion with gains alike"""
    s = ec.scene(1)
    ref16, valid, gains, _ = ec.second_round(1, **ec.BASE)
    _, opts = ec.split(ec.BASE)
    pts = s["points"].copy()
    seen = np.flatnonzero((pc.expected(1)["n_views"] > 0) & (valid > 0))
    bad = {int(seen[0]): (np.nan, 0), int(seen[len(seen) // 2]): (np.inf, 1), int(seen[len(seen) // 2 + 1]): (-np.inf, 2), int(seen[-1]): (np.nan, 2)}
    for k, (v, axis) in bad.items():
        pts[k, axis] = v
    args = (pts, s["images"], s["depth"], s["intr"], s["Rcw"], s["tcw"])
    without = valid.copy()
    without[list(bad)] = 0                                                       # the same as taking the points out
    want = eo.sums(s["points"], *args[1:], ref16, without, gains, **opts)
    got = run_sums(*args, ref16, valid, gains, **opts)
    assert same_bytes(got, want) and not same_bytes(got, ec.second_round(1, **ec.BASE)[3])
    fused = run_fuse(*args, gains=gains)
    wv, w1, w2 = eo.fuse(s["points"], *args[1:], gains)
    keep = np.ones(len(pts), bool)
    keep[list(bad)] = False
    assert not fused["n_views"][~keep].any() and same_bytes(fused["sums"][1][keep], w1[keep]) and same_bytes(fused["sums"][2][keep], w2[keep])


# ------------------------------------------------------------------------------------------------------------ 8. the pipeline
def _plain(summary):
    return {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in summary.items() if k != "ms"}


def test_run_full_pipeline_with_exposure():
    """run_full_pipeline(images=..., photo_consistency=True, exposure=True) against direct calls on the same inputs: the gains come
    from the `after` set and both sets are evaluated with them"""
    pkg, EX, PH, V, pipe = _mods()
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"], d["pairs"], d["matches"])
    out = pipe.run_full_pipeline(*args, images=images, photo_consistency=True, exposure=dict(rounds=2, min_samples=50), **cfg)
    rep = out["exposure"]
    assert sorted(out["photo_consistency"]) == sorted(out["photo_consistency_raw"]) == ["after", "before"]
    assert len(rep["mean_sigma"]) == 3 and len(rep["rounds"]) == 2 and rep["gains"].shape == (len(d["img_t"]), 3, 2)
    assert rep["options"]["min_samples"] == 50 and len(rep["status_names"]) == len(d["img_t"])
    v = out["visual"]
    sets = dict(after=(out["poses"], v["Rcw"], v["tcw"]), before=(out["poses_before"], v["Rcw_before"], v["tcw_before"]))
    with pkg.Scans([c[:, :3] for c in d["clouds"]]) as scans:
        for name, (x, Rcw, tcw) in sets.items():
            xyz, rgb, n_views, sigma = out["fused_" + name]
            assert xyz is out["colored_" + name][0] and len(xyz) > 1000
            with V.DepthImages.render(scans, x, d["times"], d["img_t"], Rcw, tcw, tp.INTR, tp.W, tp.H) as depth:
                if name == "after":
                    direct = EX.estimate_exposure(xyz, lambda k: images[k], Rcw, tcw, tp.INTR, tp.W, tp.H, depth=depth, rounds=2, min_samples=50)
                    assert same_bytes(direct["gains"], rep["gains"]) and same_bytes(direct["status"], rep["status"])
                    assert direct["mean_sigma"] == rep["mean_sigma"]
                    print("exposure", rep["mean_sigma"], rep["status_names"])
                raw = PH.photo_consistency(xyz, lambda k: images[k], Rcw, tcw, tp.INTR, tp.W, tp.H, depth=depth, chunk=3)
                comp = PH.photo_consistency(xyz, lambda k: images[k], Rcw, tcw, tp.INTR, tp.W, tp.H, depth=depth, chunk=3, gains=rep["gains"])
            assert _plain(raw["summary"]) == _plain(out["photo_consistency_raw"][name]), name
            assert _plain(comp["summary"]) == _plain(out["photo_consistency"][name]), name
            assert same_bytes(comp["rgb"], rgb) and same_bytes(comp["sigma"], sigma) and same_bytes(comp["n_views"], n_views)
    assert out["photo_consistency"]["after"]["mean_sigma"] == rep["mean_sigma"][-1]


def test_run_dataset_writes_the_report(tmp_path):
    import sqlite3
    from PIL import Image
    pkg, EX, PH, V, pipe = _mods()
    ds = importlib.import_module("global-lvba_amd.dataset")
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    root = tmp_path / "seq"
    (root / "all_pcd_body").mkdir(parents=True); (root / "all_image").mkdir()
    for t, c in zip(d["times"], d["clouds"]):
        ds.save_pcd(str(root / "all_pcd_body" / f"{t:.6f}.pcd"), np.concatenate([c[:, :3], np.zeros((len(c), 1), np.float32)], 1))
    ds.write_poses_tum(str(root / "all_pcd_body" / "lidar_poses.txt"), d["times"], d["odo"])
    for k, t in enumerate(d["img_t"]):
        Image.fromarray(np.ascontiguousarray(images[k][:, :, ::-1]), "RGB").save(root / "all_image" / f"{t:.6f}.png")
    ds.write_poses_tum(str(root / "all_image" / "image_poses.txt"), d["img_t"], d["odo"])
    con = sqlite3.connect(str(root / "colmap.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    for i, t in enumerate(d["img_t"]):
        kp4 = np.concatenate([d["kps"][i], np.ones((len(d["kps"][i]), 2), np.float32)], 1).astype(np.float32)
        con.execute("INSERT INTO images VALUES (?, ?)", (i + 1, f"{t:.6f}.png"))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (i + 1, kp4.shape[0], 4, kp4.tobytes()))
    for (i, j), m in zip(d["pairs"], d["matches"]):
        con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                    (ds.image_ids_to_pair_id(i + 1, j + 1), len(m), 2, np.asarray(m, np.uint32).tobytes()))
    con.commit(); con.close()
    out_dir = tmp_path / "out"
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir), photo_consistency=True,
                           exposure=dict(rounds=1, min_samples=50), **cfg)
    rep = json.load(open(out_dir / "exposure.json"))
    assert sorted(rep) == sorted(["gains", "gains_float", "status", "status_names", "mean_sigma", "rounds", "sums", "options"])
    assert rep["gains"] == got["exposure"]["gains"].tolist() and rep["status"] == got["exposure"]["status"].tolist()
    assert rep["mean_sigma"] == got["exposure"]["mean_sigma"] and len(rep["mean_sigma"]) == 2 and rep["options"]["min_samples"] == 50
    assert sorted(rep["options"]) == sorted(eo.DEFAULTS)
    pcj = json.load(open(out_dir / "photo_consistency.json"))
    assert sorted(pcj) == ["after", "before", "options", "raw"]
    for name in ("after", "before"):
        assert _plain(pcj[name]) == _plain(got["photo_consistency"][name]) and _plain(pcj["raw"][name]) == _plain(got["photo_consistency_raw"][name])
