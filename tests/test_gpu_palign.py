"""GPU tests of the photometric camera alignment (lvba_palign_*, csrc/palign.hip) against the numpy restatement
(tests/palign_oracle.py) on the room of tests/palign_cases.py.  n_samples compares exactly -- the fixture's margin condition,
asserted on the CPU (test_palign_host.py), is what allows that --; every fp64 sum is held to the summation bound
(3 n_samples + 64) 2^-53 sum |term| with sum |term| from the oracle: the terms are the oracle's bit for bit (the header is built
without contraction), so what differs is the order of 3 n_samples additions."""
import ctypes
import importlib
import json

import numpy as np
import pytest

import covis_cases as cc
import palign_cases as pa
import palign_oracle as pao
import photo_cases as pc

pytestmark = pytest.mark.gpu
N = cc.N_CAMERAS
CHUNK = 4096                                                                     # PAL_CHUNK of csrc/palign_device.h


def _mods():
    return (importlib.import_module("global-lvba_amd"), importlib.import_module("global-lvba_amd.palign"),
            importlib.import_module("global-lvba_amd.photo"), importlib.import_module("global-lvba_amd.visual"),
            importlib.import_module("global-lvba_amd.pipeline"))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_gpu(what, points, ref16, valid, images, depth, intr, Rcw, tcw, calls=None, n_images=None, **opts):
    """what = "linearize" or "align" on the images by calls [(first, count), ...] (default: one call): the per-image outputs in
    image order"""
    _, PA, _, V, _ = _mods()
    M = len(images) if n_images is None else n_images
    H, W = images.shape[1:3]
    dset = V.DepthImages.upload(depth) if depth is not None else None
    try:
        with PA.PhotoAligner(points, ref16, valid, M, W, H, intr, depth=dset, **opts) as al:
            parts = {}
            for a, m in (calls if calls is not None else [(0, M)]):
                parts[a] = getattr(al, what)(a, Rcw[a:a + m], tcw[a:a + m], images[a:a + m])
            keys = parts[next(iter(parts))].keys()
            return {k: np.concatenate([parts[a][k] for a in sorted(parts)]) for k in keys}
    finally:
        if dset is not None:
            dset.close()


def scene_args(size, which, with_depth=True, M=N, n=None):
    s = pc.scene(size)
    ref16, valid = pa.reference(size)
    R, t, depth = pa.poses(size, which)
    return (s["points"][:n], ref16[:n], valid[:n], s["images"][:M], depth[:M] if with_depth else None, s["intr"], R[:M], t[:M])


def assert_sums_within_bound(got, want, msg=""):
    """got [m, 31] against the oracle's list of dict(sums, abs_sums, n_samples)"""
    for j, lin in enumerate(want):
        n = lin["n_samples"]
        assert got[j, pao.CNT] == n, (msg, j, got[j, pao.CNT], n)
        bound = (3 * n + 64) * 2.0 ** -53 * lin["abs_sums"]
        bad = np.abs(got[j] - lin["sums"]) > bound
        assert not bad.any(), (msg, j, np.flatnonzero(bad), (np.abs(got[j] - lin["sums"]) / np.maximum(bound, 1e-300))[bad])


# ------------------------------------------------------------------------------------------------------- 1. linearise parity
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
@pytest.mark.parametrize("option_set", range(len(pa.OPTION_SETS)))
def test_linearize_equals_the_oracle(size, option_set):
    kw = pa.OPTION_SETS[option_set]
    with_depth, opts = pc.split(kw)
    for which in ("planted", ("turned", 0.5)):
        got = run_gpu("linearize", *scene_args(size, which, with_depth), **opts)
        want = pa.linearized(size, which, **kw)
        assert max(lin["n_samples"] for lin in want) > 100
        assert_sums_within_bound(got["sums"], want, (kw, which))
        assert same_bytes(got["n_samples"], np.array([lin["n_samples"] for lin in want], np.int64))
        assert (got["H"] == np.transpose(got["H"], (0, 2, 1))).all()


# ------------------------------------------------------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_edges(size):
    """the first 0, 1, 63, 64, 255, 256, 257 points, chunk - 1, chunk, chunk + 1 points (a workgroup owns a chunk of 4 096: the
    fixture's 4 200 points reach into a second one), all points; and the first 1, 2 and 18 images"""
    s = pc.scene(size)
    ref16, valid = pa.reference(size)
    assert CHUNK + 1 <= cc.N_PLANTED
    M = 3
    for n in (0, 1, 63, 64, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, cc.N_PLANTED):
        args = scene_args(size, ("turned", 0.5), M=M, n=n)
        got = run_gpu("linearize", *args)
        want = [pao.linearize(args[0], args[1], args[2], args[3][j], args[4][j], args[5], args[6][j], args[7][j]) for j in range(M)]
        assert got["sums"].shape == (M, 31)
        assert_sums_within_bound(got["sums"], want, f"{n} points")
        if n == 0:
            assert not got["sums"].any()
    full = pa.linearized(size, ("turned", 0.5))
    for M in (1, 2, N):
        got = run_gpu("linearize", *scene_args(size, ("turned", 0.5), M=M))
        assert_sums_within_bound(got["sums"], full[:M], f"{M} images")


# ----------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_same_bytes_for_any_batching(size):
    """one call, one image per call, reversed image order, max_batch_images 1, 2, 3 and a second run: identical bytes, of the
    linearisation's sums and of everything the iteration returns"""
    args = scene_args(size, ("turned", 0.5))
    one = [(k, 1) for k in range(N)]
    for what in ("linearize", "align"):
        ref = run_gpu(what, *args)
        for kw in (dict(), dict(calls=one), dict(calls=one[::-1]), dict(max_batch_images=1), dict(max_batch_images=2),
                   dict(max_batch_images=3), dict(calls=[(5, 13), (0, 5)], max_batch_images=3)):
            got = run_gpu(what, *args, **kw)
            for k in ref:
                assert same_bytes(got[k], ref[k]), (what, kw, k)
    # an image's result does not depend on its place: the cameras in reversed order, depth images and all
    rev = tuple(a[::-1] if i in (3, 4, 6, 7) else a for i, a in enumerate(args))
    got = run_gpu("align", *rev)
    for k in ref:
        assert same_bytes(got[k][::-1], ref[k]), k


# ----------------------------------------------------------------------------------------------------------- 4. exact cases
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_constant_colour_images_are_degenerate(size):
    """every gradient is 0: H = 0 and g = 0 exactly, the status is DEGENERATE wherever there are enough samples, and the poses come
    back bit for bit"""
    args = list(scene_args(size, ("turned", 0.5)))
    args[3] = pc.constant_images(size)[0][:N]
    lin = run_gpu("linearize", *args)
    assert not lin["H"].any() and not lin["g"].any() and lin["n_samples"].max() > 250 and (lin["sum_sq"][lin["n_samples"] > 0] > 0).all()
    got = run_gpu("align", *args)
    enough = lin["n_samples"] >= pa.MIN_SAMPLES
    assert (got["status"][enough] == pao.DEGENERATE).all() and (got["status"][~enough] == pao.TOO_FEW_SAMPLES).all()
    assert same_bytes(got["Rcw"], args[6]) and same_bytes(got["tcw"], args[7])
    assert (got["iterations"] == 1).all() and (got["accepted"] == 0).all() and same_bytes(got["rmse"], got["rmse_initial"])


def test_ramp_image_in_exact_arithmetic():
    """palign_cases.ramp_case: a 65 x 65 ramp b = x, g = y, r = x + y, R = I, fx = fy = 64 and dyadic points: gu, gv, the residuals,
    H and g follow in exact arithmetic from the formula there, so no sum rounds in any order.  Compared equal."""
    c = pa.ramp_case()
    got = run_gpu("linearize", c["points"], c["ref16"], c["valid"], c["image"], None, c["intr"], np.eye(3)[None], np.zeros((1, 3)), loss_kind=0)
    assert got["n_samples"][0] == c["n_samples"] == c["inside"].sum()
    assert same_bytes(got["H"][0], c["Hm"]) and same_bytes(got["g"][0], c["g"])
    assert got["cost"][0] == c["cost"] and got["sum_sq"][0] == c["sum_sq"] and got["sum_w"][0] == 3 * c["n_samples"]
    # the same through the Huber loss at a scale no residual reaches
    hub = run_gpu("linearize", c["points"], c["ref16"], c["valid"], c["image"], None, c["intr"], np.eye(3)[None], np.zeros((1, 3)), loss_scale=2.0)
    assert same_bytes(hub["sums"], got["sums"])


# --------------------------------------------------------------------------------------------------------------- 5. alignment
def gpu_spread(size, Rcw, tcw, depth):
    _, _, PH, V, _ = _mods()
    s = pc.scene(size)
    with V.DepthImages.upload(depth) as dset:
        return PH.photo_consistency(s["points"], s["images"][:N], Rcw, tcw, s["intr"], s["W"], s["H"], depth=dset)["summary"]["mean_sigma"]


@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_alignment_against_the_oracle(size):
    """statuses equal the oracle's; refused cameras come back bit for bit; at 160 x 128 every accepted camera is within twice the
    oracle's own error of the truth (twice: an accept / reject decision may branch on the last bits of a tree sum); the device's
    poses are within 1e-6 (rad, m) of the oracle's; the fusion's mean spread at the returned cameras is below the spread at the start"""
    s = pc.scene(size)
    e = pa.aligned(size, 0.5, 1)[0]
    R0, t0, depth = e["start"]
    got = run_gpu("align", *scene_args(size, ("turned", 0.5)))
    assert same_bytes(got["status"], e["status"].astype(np.int32)), (got["status"], e["status"])
    refused = got["status"] == pao.TOO_FEW_SAMPLES
    assert 0 < refused.sum() < N
    assert same_bytes(got["Rcw"][refused], R0[refused]) and same_bytes(got["tcw"][refused], t0[refused])
    assert (got["iterations"][refused] == 1).all() and same_bytes(got["n_samples"], e["n_samples"].astype(np.int64))
    rot, centre = pao.pose_errors(got["Rcw"], got["tcw"], s["Rcw"][:N], s["tcw"][:N])
    dR, dt = np.abs(got["Rcw"] - e["Rcw"]).max(), np.abs(got["tcw"] - e["tcw"]).max()
    print(f"size {cc.SIZES[size]}: accepted cameras: worst rotation {rot[~refused].max():.4f} deg, worst centre "
          f"{1e3 * centre[~refused].max():.2f} mm; device minus oracle: {dR:.2e} (rotation entries), {dt:.2e} m; passes "
          f"{got['iterations'][~refused].tolist()}, accepted {got['accepted'][~refused].tolist()}")
    assert (0, 0.5, 1) in pa.ORACLE_WORST                                       # the accuracy claim is the larger size's (palign_cases.py)
    if size == 0:
        w_rot, w_centre = pa.ORACLE_WORST[0, 0.5, 1]
        assert rot[~refused].max() <= 2 * w_rot and centre[~refused].max() <= 2 * w_centre
    assert dR <= 1e-6 and dt <= 1e-6
    assert (got["rmse"][~refused] < got["rmse_initial"][~refused]).all()
    assert np.allclose(got["rmse"], e["rmse"], rtol=0, atol=1e-6) and np.allclose(got["rmse_initial"], e["rmse_initial"], rtol=1e-12, atol=0)
    assert (got["information"] == np.transpose(got["information"], (0, 2, 1))).all() and (got["information"][~refused, 0, 0] > 0).all()
    before = gpu_spread(size, R0, t0, depth)
    after = gpu_spread(size, got["Rcw"], got["tcw"], pa.rerendered(size, got["Rcw"], got["tcw"]))
    print(f"size {cc.SIZES[size]}: mean spread {before:.3f} -> {after:.3f}")
    assert after < before


LOOSE = dict(eps_rot=1e-3, eps_trans=1e-2)                                      # thresholds the iteration reaches within its passes


@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_converged_images_leave_the_lock_step_early(size):
    """eps_rot = 1e-3, eps_trans = 1e-2: the oracle ends the accepted cameras CONVERGED after 3 or 4 passes (at 37 x 29 one of them
    still runs to MAX_ITERATIONS beside them); the device gives the same statuses, passes and accepted steps and the oracle's poses,
    the finished images are skipped by the later passes, and a batch whose images have all finished stops before max_iterations"""
    e = pa.aligned(size, 0.5, 1, **LOOSE)[0]
    conv = e["status"] == pao.CONVERGED
    assert conv.sum() >= 10 and (e["iterations"][conv] < pao.DEFAULTS["max_iterations"]).all() and (e["accepted"][conv] >= 1).all()
    args = scene_args(size, ("turned", 0.5))
    got = run_gpu("align", *args, **LOOSE)
    assert same_bytes(got["status"], e["status"].astype(np.int32)), (got["status"], e["status"])
    assert same_bytes(got["iterations"], e["iterations"].astype(np.int32)) and same_bytes(got["accepted"], e["accepted"].astype(np.int32))
    assert np.abs(got["Rcw"] - e["Rcw"]).max() <= 1e-6 and np.abs(got["tcw"] - e["tcw"]).max() <= 1e-6
    assert np.allclose(got["rmse"], e["rmse"], rtol=0, atol=1e-6) and (got["rmse"][conv] < got["rmse_initial"][conv]).all()
    # an image converges on its own, whatever runs beside it: one image per call, and batches of two
    one = run_gpu("align", *args, calls=[(k, 1) for k in range(N)], **LOOSE)
    two = run_gpu("align", *args, max_batch_images=2, **LOOSE)
    for k in got:
        assert same_bytes(one[k], got[k]) and same_bytes(two[k], got[k]), k


def test_out_of_bounds_and_the_pass_limit():
    """max_rotation_deg below the planted turn: OUT_OF_BOUNDS, the initial pose back bit for bit with the initial pose's figures;
    max_iterations = 1: one pass, MAX_ITERATIONS, the pose unchanged"""
    args = scene_args(0, ("turned", 0.5))
    e = pa.aligned(0, 0.5, 1)[0]
    enough = e["status"] != pao.TOO_FEW_SAMPLES
    got = run_gpu("align", *args, max_rotation_deg=0.1)
    assert (got["status"][enough] == pao.OUT_OF_BOUNDS).all() and (got["status"][~enough] == pao.TOO_FEW_SAMPLES).all()
    assert same_bytes(got["Rcw"], args[6]) and same_bytes(got["tcw"], args[7])
    assert same_bytes(got["rmse"], got["rmse_initial"]) and (got["accepted"][enough] >= 1).all()
    got = run_gpu("align", *args, max_translation=1e-4)
    assert (got["status"][enough] == pao.OUT_OF_BOUNDS).all() and same_bytes(got["Rcw"], args[6])
    got = run_gpu("align", *args, max_iterations=1)
    assert (got["status"][enough] == pao.MAX_ITERATIONS).all() and (got["iterations"] == 1).all()
    assert same_bytes(got["Rcw"], args[6]) and same_bytes(got["tcw"], args[7])


# --------------------------------------------------------------------------------------------------------------- 6. refusals
def test_invalid_arguments_are_refused():
    pkg, PA, _, V, _ = _mods()
    L = pkg._lib
    lib = ctypes.CDLL(L.LIB_PATH)                           # raw prototypes: NULL pointers go through as they are
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.lvba_palign_create.argtypes = [i32, i64, vp, vp, vp, i32, i32, i32, vp, vp, vp, ctypes.POINTER(vp)]
    lib.lvba_palign_linearize.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.lvba_palign_align.argtypes = [vp, i32, i32, vp, vp, vp] + [vp] * 10
    lib.lvba_palign_profile.argtypes = [vp, vp]
    lib.lvba_palign_free.argtypes = [vp]
    lib.lvba_palign_free.restype = None
    lib.lvba_last_error.restype = ctypes.c_char_p
    s = pc.scene(1)
    W, H, M = s["W"], s["H"], N
    ptr = lambda a: a.ctypes.data if a is not None else None
    pts, intr = s["points"], np.ascontiguousarray(s["intr"])
    ref16, valid = pa.reference(1)
    n = len(pts)
    SENTINEL = 0x5A5A
    h = vp(SENTINEL)

    def create(dev=0, n=n, P=pts, F=ref16, K=valid, M=M, w=W, hh=H, I=intr, depth=None, out=True, **o):
        h.value = SENTINEL
        opts = PA.palign_opts() if o else None
        for k, v in o.items():
            setattr(opts, k, v)                                                  # past make_opts' coercion: NaN, negatives
        return lib.lvba_palign_create(dev, n, ptr(P), ptr(F), ptr(K), M, w, hh, ptr(I), depth,
                                      ctypes.byref(opts) if opts is not None else None, ctypes.byref(h) if out else None)

    def refused(rc):
        return rc == L.ERR_ARG and h.value == SENTINEL                           # nothing written

    assert refused(create(P=None)) and refused(create(F=None)) and refused(create(K=None)) and refused(create(I=None))
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
    for name in ("occlusion_rel", "occlusion_abs", "max_depth", "eps_rot", "eps_trans", "max_rotation_deg", "max_translation"):
        for v in (-1e-3, np.nan, np.inf):
            assert refused(create(**{name: v})), (name, v)
    for v in (0.0, -1.0, np.nan, np.inf):
        assert refused(create(loss_scale=v)), v
    assert refused(create(loss_kind=-1)) and refused(create(loss_kind=6))
    assert refused(create(max_iterations=0)) and refused(create(max_iterations=1001))
    assert refused(create(min_samples=5)) and refused(create(max_batch_images=-1))
    with V.DepthImages.upload(s["depth"][:5]) as few, V.DepthImages.upload(pc.scene(0)["depth"][:M]) as other_size:
        assert refused(create(depth=few._h)) and refused(create(depth=other_size._h))
        assert b"depth set" in lib.lvba_last_error()
    R, t, depth = pa.poses(1, ("turned", 0.5))
    img = s["images"][:M]
    e = pa.linearized(1, ("turned", 0.5))
    with V.DepthImages.upload(depth) as dset:
        assert create(depth=dset._h, min_samples=6, max_iterations=1000) == L.OK and h.value not in (None, SENTINEL)
        lib.lvba_palign_free(h)
        assert create(depth=dset._h) == L.OK and h.value not in (None, SENTINEL)
        SENT = 7.25
        sums = np.full((M, 31), SENT)
        outs = [np.full((M, 9), SENT), np.full((M, 3), SENT), np.full(M, 7, np.int32), np.full(M, 7, np.int32), np.full(M, 7, np.int32),
                np.full(M, 7, np.int64), np.full(M, SENT), np.full(M, SENT), np.full(M, SENT), np.full((M, 36), SENT)]
        untouched = lambda: (sums == SENT).all() and all((o == (SENT if o.dtype == np.float64 else 7)).all() for o in outs)

        def lin(first, m, R=R, t=t, img=img, hh=h, out=sums):
            return lib.lvba_palign_linearize(hh, first, m, ptr(R), ptr(t), ptr(img), ptr(out))

        def ali(first, m, R=R, t=t, img=img, hh=h, drop=None):
            o = [None if k == drop else ptr(a) for k, a in enumerate(outs)]
            return lib.lvba_palign_align(hh, first, m, ptr(R), ptr(t), ptr(img), *o)

        for f in (lin, ali):
            assert f(0, 1, hh=None) == L.ERR_ARG
            assert f(-1, 2) == L.ERR_ARG and f(0, -1) == L.ERR_ARG and f(M, 1) == L.ERR_ARG and f(M - 1, 2) == L.ERR_ARG
            assert f(0, 2, R=None) == L.ERR_ARG and f(0, 2, t=None) == L.ERR_ARG and f(0, 2, img=None) == L.ERR_ARG
            badR = R.copy(); badR[1, 0, 0] = np.nan
            assert f(0, 2, R=badR) == L.ERR_ARG and b"camera 1: non-finite rotation" in lib.lvba_last_error()
            badt = t.copy(); badt[0, 2] = np.inf
            assert f(0, 2, t=badt) == L.ERR_ARG and b"non-finite translation" in lib.lvba_last_error()
            assert untouched()
        assert lin(0, 2, out=None) == L.ERR_ARG
        for k in range(len(outs)):
            assert ali(0, 2, drop=k) == L.ERR_ARG, k
        assert untouched()
        assert lib.lvba_palign_profile(None, ptr(np.zeros(3))) == L.ERR_ARG and lib.lvba_palign_profile(h, None) == L.ERR_ARG
        assert lin(0, 0) == L.OK and ali(0, 0) == L.OK and untouched()           # no image: nothing to write
        assert lin(0, M) == L.OK                                                 # the handle is still usable
        assert_sums_within_bound(sums, e, "after the refusals")
        ms = np.zeros(3)
        assert lib.lvba_palign_profile(h, ptr(ms)) == L.OK and ms[1] > 0 and (ms >= 0).all()
        lib.lvba_palign_free(h)
        lib.lvba_palign_free(None)
    assert pkg._lib.load().lvba_version() == 112
    with pytest.raises(TypeError):
        PA.PhotoAligner(pts, ref16, valid, M, W, H, intr, no_such_option=1)
    with pytest.raises(ValueError):
        PA.PhotoAligner(pts, ref16[:5], valid, M, W, H, intr)


def test_non_finite_and_invalid_points_are_never_sampled():
    args = list(scene_args(1, "planted"))
    base = run_gpu("linearize", *args)
    s = pc.scene(1)
    rec = [pao.records(args[0], args[1], args[2], args[3][j], args[4][j], args[5], args[6][j], args[7][j])["seen"] for j in range(N)]
    often = np.argsort(-np.sum(rec, 0))[:6]                                      # the points most cameras sample
    pts, valid = args[0].copy(), args[2].copy()
    pts[often[0], 0], pts[often[1], 1], pts[often[2], 2], pts[often[3], 0] = np.nan, np.inf, -np.inf, np.nan
    valid[often[4]] = valid[often[5]] = 0
    args[0], args[2] = pts, valid
    got = run_gpu("linearize", *args)
    gone = np.sum(np.asarray(rec)[:, often], 1)
    assert gone.max() >= 4 and same_bytes(got["n_samples"], base["n_samples"] - gone)
    want = [pao.linearize(pts, args[1], valid, args[3][j], args[4][j], args[5], args[6][j], args[7][j]) for j in range(N)]
    assert_sums_within_bound(got["sums"], want, "non-finite and invalid points")
    assert s["points"] is not pts


# --------------------------------------------------------------------------------------------------------------- 7. the pipeline
def test_align_cameras_photometric_on_the_room():
    """the pipeline's rounds on the room, reference fused from the turned cameras themselves (the colour-map optimisation): the
    spread falls from round to round; the report has one status per image and rounds + 1 spreads"""
    _, PA, _, V, pipe = _mods()
    s = pc.scene(0)
    R0, t0, depth = pa.poses(0, ("turned", 0.5))
    render = lambda Rk, tk: V.DepthImages.upload(pa.rerendered(0, Rk, tk))
    with V.DepthImages.upload(depth) as dset:
        rep = pipe.align_cameras_photometric(s["points"], s["images"][:N], (R0, t0), dset, s["intr"], s["W"], s["H"], rounds=2, render=render,
                                             chunk=5)
    print("mean spread per round:", rep["mean_sigma"], "statuses:", rep["status_names"])
    assert len(rep["mean_sigma"]) == 3 and rep["mean_sigma"][2] < rep["mean_sigma"][1] < rep["mean_sigma"][0]
    assert len(rep["rounds"]) == 2 and rep["status"].shape == (N,) and rep["Rcw"].shape == (N, 3, 3)
    assert rep["options"]["min_samples"] == 200 and set(rep["status_names"]) <= set(PA.STATUS.values())
    moved = rep["status"] != PA.TOO_FEW_SAMPLES
    assert moved.any() and same_bytes(rep["Rcw"][~moved], R0[~moved])


def test_run_full_pipeline_with_photo_align(tmp_path):
    """photo_align=True on the sequence of test_gpu_colorize.py equals a direct align_cameras_photometric call on the same inputs;
    "apply" changes fused_after (and its summary) and nothing else; run_dataset writes photo_align.json"""
    pkg, PA, PH, V, pipe = _mods()
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"], d["pairs"], d["matches"])
    opts = dict(min_samples=50)
    out = pipe.run_full_pipeline(*args, images=images, photo_consistency=True, photo_align=dict(opts), **cfg)
    rep = out["photo_align"]
    print("photo_align:", rep["status_names"], rep["mean_sigma"])
    v = out["visual"]
    with pkg.Scans([c[:, :3] for c in d["clouds"]]) as scans:
        render = lambda Rk, tk: V.DepthImages.render(scans, out["poses"], d["times"], d["img_t"], Rk, tk, tp.INTR, tp.W, tp.H)
        with render(v["Rcw"], v["tcw"]) as depth:
            direct = pipe.align_cameras_photometric(out["colored_after"][0], images, (v["Rcw"], v["tcw"]), depth, tp.INTR, tp.W, tp.H,
                                                    render=render, **opts)
    assert same_bytes(direct["Rcw"], out["photo_align_cameras"][0]) and same_bytes(direct["tcw"], out["photo_align_cameras"][1])
    for k in ("status", "iterations", "accepted", "n_samples", "rmse_initial", "rmse", "cost"):
        assert same_bytes(direct[k], rep[k]), k
    assert json.dumps(direct["mean_sigma"]) == json.dumps(rep["mean_sigma"]) and rep["applied"] is False and len(rep["mean_sigma"]) == 2
    app = pipe.run_full_pipeline(*args, images=images, photo_consistency=True, photo_align=dict(opts, apply=True), **cfg)
    assert app["photo_align"]["applied"] is True and same_bytes(app["photo_align_cameras"][0], out["photo_align_cameras"][0])
    for k in ("poses", "poses_before"):
        assert same_bytes(app[k], out[k]), k
    for k in ("Rcw", "tcw", "Rcw_before", "tcw_before"):
        assert same_bytes(app["visual"][k], v[k]), k
    for k in ("colored_after", "colored_before", "fused_before"):
        assert all(same_bytes(a, b) for a, b in zip(app[k], out[k])), k
    moved = np.isin(rep["status"], (PA.CONVERGED, PA.MAX_ITERATIONS)) & (rep["accepted"] > 0)
    assert moved.any()                                                           # a condition on the sequence: some camera did move
    assert not same_bytes(out["photo_align_cameras"][0], v["Rcw"])
    assert not all(same_bytes(a, b) for a, b in zip(app["fused_after"], out["fused_after"]))
    plain = lambda q: {k: x for k, x in q.items() if k != "ms"}
    assert plain(app["photo_consistency"]["before"]) == plain(out["photo_consistency"]["before"])
    assert plain(app["photo_consistency"]["after"]) != plain(out["photo_consistency"]["after"])


def test_run_dataset_writes_the_report(tmp_path):
    import sqlite3
    from PIL import Image
    pkg, PA, PH, V, pipe = _mods()
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
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir), photo_align=dict(min_samples=50), **cfg)
    rep = json.load(open(out_dir / "photo_align.json"))
    assert rep["status"] == got["photo_align"]["status"].tolist() and rep["status_names"] == got["photo_align"]["status_names"]
    assert rep["options"]["min_samples"] == 50 and sorted(rep["options"]) == sorted(pao.DEFAULTS) and rep["applied"] is False
    assert len(rep["mean_sigma"]) == 2 and len(rep["rmse"]) == len(d["img_t"]) and len(rep["rounds"]) == 1
    assert not (out_dir / "colored_merged_after.pcd").exists() and not (out_dir / "photo_consistency.json").exists()
