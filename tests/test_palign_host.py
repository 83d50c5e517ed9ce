"""CPU tests of the photometric camera alignment (include/lvba_hip.h "photometric camera alignment against the coloured map",
DESIGN.md §10q): the device header compiled for the host against the numpy oracle bit for bit, the oracle's Jacobian against
differences, its integer gradient against plain loops, the 6 x 6 LDL^T against numpy, the fixture's conditions and the claim -- the
oracle brings every camera with enough samples back to the truth and lowers the spread --, and the binding's mirrors."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import covis_cases as cc
import covis_oracle as co
import match_cases as mc
import palign_cases as pa
import palign_oracle as pao
import photo_cases as pc
from host_build import build_check

N = cc.N_CAMERAS
POSES = ("planted", ("turned", 0.5))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/palign_device.h compiled for the host, without contraction (tests/palign_check.cpp)"""
    lib = ctypes.CDLL(build_check("palign_check", tmp_path_factory.mktemp("emul_palign")))
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emul_records.argtypes = [ctypes.c_int64, P, P, P, I, I, P, P, P, P, P, P, P] + [P] * 9
    lib.emul_gradient.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.c_uint32] * 4 + [I, P, P]
    lib.emul_jpi.argtypes = [P, P, P, P]
    lib.emul_project_cam.argtypes = [P, P, P]
    lib.emul_solve.argtypes = [P, D, P]
    lib.emul_retract.argtypes = [P] * 5
    lib.emul_align.argtypes = [ctypes.c_int64, P, P, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.emul_records.restype = lib.emul_gradient.restype = lib.emul_jpi.restype = lib.emul_retract.restype = lib.emul_align.restype = None
    return lib


def ptr(x):
    return x.ctypes.data


def rule_arrays(**kw):
    o = dict(pao.DEFAULTS, **kw)
    return (np.array([o["occlusion_rel"], o["occlusion_abs"], o["max_depth"], o["loss_scale"]], np.float64),
            np.array([o["holes"], o["loss_kind"]], np.int32), o)


def host_records(emul, points, ref16, valid, image, depth, intr, R, t, **kw):
    bounds, flags, _ = rule_arrays(**kw)
    n = len(points)
    H, W = image.shape[:2]
    out = dict(seen=np.zeros(n, np.uint8), c16=np.zeros((n, 3), np.int32), gu=np.zeros((n, 3)), gv=np.zeros((n, 3)), r=np.zeros((n, 3)),
               J=np.zeros((n, 3, 6)), rho=np.zeros((n, 3)), w=np.zeros((n, 3)), sums=np.zeros(pao.NS))
    R, t = np.ascontiguousarray(R, np.float64), np.ascontiguousarray(t, np.float64)
    emul.emul_records(n, ptr(points), ptr(ref16), ptr(valid), W, H, None if depth is None else ptr(depth), ptr(R), ptr(t), ptr(image),
                      ptr(np.ascontiguousarray(intr, np.float64)), ptr(bounds), ptr(flags),
                      *(ptr(out[k]) for k in ("seen", "c16", "gu", "gv", "r", "J", "rho", "w", "sums")))
    return out


def host_align(emul, points, ref16, valid, image, depth, intr, R, t, **kw):
    bounds, flags, o = rule_arrays(**kw)
    half = 0.5 * math.radians(o["max_rotation_deg"])
    par = np.array([o["loss_scale"], o["eps_rot"], o["eps_trans"], 8.0 * math.sin(half) * math.sin(half), o["max_translation"]])
    ipar = np.array([o["loss_kind"], o["min_samples"], o["max_iterations"]], np.int32)
    oi, od = np.zeros(3, np.int32), np.zeros(12 + 2 * pao.NS)
    H, W = image.shape[:2]
    R, t = np.ascontiguousarray(R, np.float64), np.ascontiguousarray(t, np.float64)
    emul.emul_align(len(points), ptr(points), ptr(ref16), ptr(valid), W, H, None if depth is None else ptr(depth), ptr(R), ptr(t), ptr(image),
                    ptr(np.ascontiguousarray(intr, np.float64)), ptr(bounds), ptr(flags), ptr(par), ptr(ipar), ptr(oi), ptr(od))
    return dict(status=int(oi[0]), iterations=int(oi[1]), accepted=int(oi[2]), Rcw=od[:9].reshape(3, 3), tcw=od[9:12],
                cur=od[12:12 + pao.NS], first=od[12 + pao.NS:])


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. header == oracle, bit for bit
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_device_header_on_the_host_equals_the_oracle(emul, size):
    """c16, gu, gv, residuals, the 6-vector rows and the weights of every sample: both sizes, planted and turned poses, with and
    without the depth set"""
    s = pc.scene(size)
    ref16, valid = pa.reference(size)
    n_records = 0
    for which in POSES:
        R, t, depth = pa.poses(size, which)
        for with_depth in (True, False):
            for j in range(N):
                d = depth[j] if with_depth else None
                e = pao.records(s["points"], ref16, valid, s["images"][j], d, s["intr"], R[j], t[j])
                g = host_records(emul, s["points"], ref16, valid, s["images"][j], d, s["intr"], R[j], t[j])
                assert same_bytes(g["seen"].astype(bool), e["seen"]), (which, with_depth, j)
                i = e["index"]
                assert same_bytes(g["c16"][i].astype(np.int64), e["c16"]), (which, with_depth, j)
                for k in ("gu", "gv", "r", "J", "rho", "w"):
                    assert same_bytes(g[k][i], e[k]), (which, with_depth, j, k)
                n_records += len(i)
                # the header's own sums (a walk in index order) against the oracle's pairwise ones: the summation bound
                es, ea = pao.sums_of(e)
                assert g["sums"][pao.CNT] == es[pao.CNT] == len(i)
                assert (np.abs(g["sums"] - es) <= (3 * len(i) + 64) * 2.0 ** -53 * ea).all(), (which, with_depth, j)
    assert n_records > 5000


def test_invalid_and_non_finite_points_are_never_sampled(emul):
    s = pc.scene(1)
    ref16, valid = pa.reference(1)
    R, t, depth = pa.poses(1, "planted")
    base = pao.records(s["points"], ref16, valid, s["images"][0], depth[0], s["intr"], R[0], t[0])
    pts, ok = s["points"].copy(), valid.copy()
    i = base["index"]
    pts[i[0], 0], pts[i[1], 1], pts[i[2], 2], ok[i[3]] = np.nan, np.inf, -np.inf, 0
    for f in (lambda *a: pao.records(*a), lambda *a: host_records(emul, *a)):
        got = f(pts, ref16, ok, s["images"][0], depth[0], s["intr"], R[0], t[0])
        seen = np.asarray(got["seen"]).astype(bool)
        assert not seen[i[:4]].any() and seen[i[4:]].all() and seen.sum() == len(i) - 4


# ------------------------------------------------------------------------------------------------------------ 2. the Jacobian
def test_projection_jacobian_against_central_differences(emul):
    """Jpi of the header and of the oracle against central differences of trk_project_cam, 1e-6 relative, distortion included"""
    rng = np.random.default_rng(3)
    intr = np.array([420.0, 410.0, 321.5, 243.25, -0.21, 0.07, 1.3e-3, -0.8e-3])
    Xc = np.stack([rng.uniform(-1.5, 1.5, 200), rng.uniform(-1.2, 1.2, 200), rng.uniform(2.0, 6.0, 200)], 1)
    Ju, Jv = pao.jpi(intr, Xc)
    for i in range(len(Xc)):
        hu, hv = np.zeros(3), np.zeros(3)
        emul.emul_jpi(ptr(intr), ptr(np.ascontiguousarray(Xc[i])), ptr(hu), ptr(hv))
        assert same_bytes(hu, Ju[i]) and same_bytes(hv, Jv[i])
        for a in range(3):
            h = 1e-6 * max(1.0, abs(Xc[i, a]))
            lo, hi, p, q = Xc[i].copy(), Xc[i].copy(), np.zeros(2), np.zeros(2)
            lo[a] -= h; hi[a] += h
            assert emul.emul_project_cam(ptr(intr), ptr(lo), ptr(p)) and emul.emul_project_cam(ptr(intr), ptr(hi), ptr(q))
            d = (q - p) / (hi[a] - lo[a])
            scale = max(np.abs(Ju[i]).max(), np.abs(Jv[i]).max())
            assert abs(d[0] - Ju[i, a]) <= 1e-6 * scale and abs(d[1] - Jv[i, a]) <= 1e-6 * scale, (i, a)


def bilinear(image, u, v, k):
    """the bilinear sample of channel k with the exact fractions (no 1/256 quantisation), in grey levels"""
    x, y = int(math.floor(u)), int(math.floor(v))
    fu, fv = u - x, v - y
    t = image.astype(np.float64)
    return (1 - fu) * (1 - fv) * t[y, x, k] + fu * (1 - fv) * t[y, x + 1, k] + (1 - fu) * fv * t[y + 1, x, k] + fu * fv * t[y + 1, x + 1, k]


def test_row_against_differences_of_the_bilinear_sample():
    """away from texel edges: (a) the gradient with the fractions quantised to 1/256 differs from the exact bilinear gradient by at
    most |t11 - t10 - t01 + t00| / 256; (b) the row built with the exact gradient equals central differences of the bilinear sample
    under the left perturbation, to 1e-5 of the row's largest entry"""
    s = pc.scene(0)
    ref16, valid = pa.reference(0)
    R, t, depth = pa.poses(0, "planted")
    j = 0
    e = pao.records(s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j])
    fu, fv = e["u"] - np.floor(e["u"]), e["v"] - np.floor(e["v"])
    pick = np.flatnonzero((fu > 0.2) & (fu < 0.8) & (fv > 0.2) & (fv < 0.8))[:40]
    assert len(pick) == 40
    img = s["images"][j]
    X = s["points"].astype(np.float64)[e["index"]]
    Xc = pao.camera_points(R[j], t[j], X)
    Ju, Jv = pao.jpi(s["intr"], Xc)
    for i in pick:
        x, y = int(e["u"][i]), int(e["v"][i])
        for k in range(3):
            t00, t10, t01, t11 = (float(img[y, x, k]), float(img[y, x + 1, k]), float(img[y + 1, x, k]), float(img[y + 1, x + 1, k]))
            gu = (1 - fv[i]) * (t10 - t00) + fv[i] * (t11 - t01)
            gv = (1 - fu[i]) * (t01 - t00) + fu[i] * (t11 - t10)
            mixed = abs(t11 - t10 - t01 + t00)
            assert abs(e["gu"][i, k] - gu) <= mixed / 256 + 1e-12 and abs(e["gv"][i, k] - gv) <= mixed / 256 + 1e-12
            q = gu * Ju[i] + gv * Jv[i]
            row = np.r_[np.cross(Xc[i], q), q]
            for a in range(6):
                h = 1e-6
                vals = []
                for sgn in (-1.0, 1.0):
                    d = np.zeros(6); d[a] = sgn * h
                    Rn, tn = pao.retract(R[j].reshape(9), t[j], d)
                    u, v, _, ok = co.project(s["intr"], Rn.reshape(3, 3), tn, X[i:i + 1])
                    assert ok[0] and int(u[0]) == x and int(v[0]) == y
                    vals.append(bilinear(img, float(u[0]), float(v[0]), k))
                assert abs((vals[1] - vals[0]) / (2 * h) - row[a]) <= 1e-5 * max(np.abs(row).max(), 1.0), (i, k, a)
            # and the oracle's own row is this row with the quantised gradient
            qq = e["gu"][i, k] * Ju[i] + e["gv"][i, k] * Jv[i]
            assert np.allclose(e["J"][i, k], np.r_[np.cross(Xc[i], qq), qq], rtol=1e-12, atol=1e-12)


def test_gradient_numerators_against_plain_loops(emul):
    """the oracle's and the header's integer numerators and c16 against Python integers, on the room and on random texels"""
    s = pc.scene(1)
    ref16, valid = pa.reference(1)
    R, t, depth = pa.poses(1, ("turned", 0.5))
    for j in (0, 5, 11):
        e = pao.records(s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j])
        for i in range(0, len(e["index"]), 7):
            for k in range(3):
                nu, nv, c16 = pao.loops_gradient(s["images"][j], float(e["u"][i]), float(e["v"][i]), k)
                assert e["gu"][i, k] == nu / 256.0 and e["gv"][i, k] == nv / 256.0 and e["c16"][i, k] == c16
    rng = np.random.default_rng(4)
    for _ in range(300):
        a, b = (int(x) for x in rng.integers(0, 256, 2))
        tex = rng.integers(0, 256, (4, 3))
        tex[:, 0] = rng.choice([0, 255], 4)                                      # the extremes: |numerator| up to 255 * 256
        words = [int(tx[0]) | int(tx[1]) << 8 | int(tx[2]) << 16 for tx in tex]
        for k in range(3):
            nu, nv = ctypes.c_int32(), ctypes.c_int32()
            emul.emul_gradient(a, b, *words, k, ctypes.byref(nu), ctypes.byref(nv))
            t00, t10, t01, t11 = (int(tex[q, k]) for q in range(4))
            assert nu.value == (256 - b) * (t10 - t00) + b * (t11 - t01) and nv.value == (256 - a) * (t01 - t00) + a * (t11 - t10)
            on, ov = pao.gradient_numerators(np.array([a]), np.array([b]), *(tex[q:q + 1] for q in range(4)))
            assert on[0, k] == nu.value and ov[0, k] == nv.value


# ------------------------------------------------------------------------------------------------------------- 3. the solve
def test_ldlt_matches_numpy_solve_on_the_fixtures_own_systems(emul):
    """pal_solve of the header and of the oracle against numpy.linalg.solve, 1e-12 relative, at the damping values the iteration
    visits; the two agree with each other bit for bit"""
    worst = 0.0
    for size in range(len(cc.SIZES)):
        for lin in pa.linearized(size, ("turned", 0.5)):
            if lin["n_samples"] < pa.MIN_SAMPLES:
                continue
            s = lin["sums"]
            H = pao.expand(s)
            for lam in (pao.LAMBDA_MIN, pao.LAMBDA0 / 3, pao.LAMBDA0, 4 * pao.LAMBDA0, 4.0 ** 8 * pao.LAMBDA0):
                d = np.zeros(6)
                assert emul.emul_solve(ptr(np.ascontiguousarray(s)), lam, ptr(d)) == 1
                assert same_bytes(d, pao.solve(s, lam))
                want = np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), pao.DIAG_FLOOR)), -s[pao.G0:pao.G0 + 6])
                worst = max(worst, np.abs(d - want).max() / np.abs(want).max())
    print(f"worst relative difference to numpy.linalg.solve: {worst:.2e}")
    assert worst <= 1e-12
    bad = np.zeros(pao.NS)
    bad[0] = -1.0
    assert emul.emul_solve(ptr(bad), 1e-3, ptr(np.zeros(6))) == 0 and pao.solve(bad, 1e-3) is None


def test_retraction_equals_the_oracles(emul):
    rng = np.random.default_rng(5)
    s = pc.scene(0)
    for j in range(6):
        d = rng.normal(size=6) * 1e-2
        Rn, tn = np.zeros(9), np.zeros(3)
        R, t = np.ascontiguousarray(s["Rcw"][j].reshape(9)), np.ascontiguousarray(s["tcw"][j])
        emul.emul_retract(ptr(R), ptr(t), ptr(d), ptr(Rn), ptr(tn))
        eR, et = pao.retract(R, t, d)
        assert same_bytes(Rn, eR) and same_bytes(tn, et)
        assert np.abs(Rn.reshape(3, 3) @ Rn.reshape(3, 3).T - np.eye(3)).max() < 1e-15


# --------------------------------------------------------------------------------------------------- 4. the fixture's conditions
def test_fixture_conditions_at_the_given_poses():
    """the fusion's margins hold at every pose the parity tests linearise at (the linearisation takes no decision on min_samples;
    check_alignment below holds every pose the iteration visits MIN_GAP away from it)"""
    for size in range(len(cc.SIZES)):
        for which in POSES:
            for kw in pa.OPTION_SETS:
                for lin in pa.linearized(size, which, **kw):
                    m = lin["margins"]
                    assert m["compare"] >= mc.MIN_MARGIN and m["texel"] >= pc.TEXEL_MARGIN, (size, which, kw, m)
    counts = [[lin["n_samples"] for lin in pa.linearized(0, "planted", **kw)] for kw in pa.OPTION_SETS]
    assert len({tuple(c) for c in counts}) >= 3      # the sets sample different things (none of the 18 cameras' depth images has holes)


def check_alignment(size, degrees, rounds):
    out = pa.aligned(size, degrees, rounds)
    s = pc.scene(size)
    for k, r in enumerate(out):
        assert r["margins"]["compare"] >= mc.MIN_MARGIN and r["margins"]["texel"] >= pc.TEXEL_MARGIN, (size, degrees, k, r["margins"])
        assert r["min_gap"] >= pa.MIN_GAP
        few = np.array([lin["n_samples"] for lin in [pao.linearize(s["points"], *pa.reference(size), s["images"][j], r["start"][2][j],
                                                                   s["intr"], r["start"][0][j], r["start"][1][j]) for j in range(N)]])
        assert ((r["status"] == pao.TOO_FEW_SAMPLES) == (few < pa.MIN_SAMPLES)).all()          # exactly the cameras below the threshold
        refused = r["status"] == pao.TOO_FEW_SAMPLES
        assert same_bytes(r["Rcw"][refused], r["start"][0][refused]) and same_bytes(r["tcw"][refused], r["start"][1][refused])
        assert np.isin(r["status"][~refused], (pao.CONVERGED, pao.MAX_ITERATIONS)).all()
    last = out[-1]
    ok = last["status"] != pao.TOO_FEW_SAMPLES
    print(f"size {cc.SIZES[size]}, turned {degrees} deg, {rounds} round(s): {int((~ok).sum())} of {N} refused; accepted cameras: worst "
          f"rotation {last['rot_err'][ok].max():.4f} deg (median {np.median(last['rot_err'][ok]):.4f}), worst centre "
          f"{1e3 * last['centre_err'][ok].max():.2f} mm (median {1e3 * np.median(last['centre_err'][ok]):.2f}); rmse "
          f"{np.median(last['rmse_initial'][ok]):.2f} -> {np.median(last['rmse'][ok]):.2f} grey levels")
    return last, ok


def test_the_oracle_brings_every_camera_with_enough_samples_back():
    """160 x 128, reference = the planted colours, turned(0, 0.5, 7): the oracle refuses exactly the cameras below min_samples and
    leaves every other one within ORACLE_WORST of the truth, itself within the issue's 0.1 degrees and 1 cm; likewise at 2 degrees
    with two rounds"""
    for degrees, rounds in ((0.5, 1), (2.0, 2)):
        last, ok = check_alignment(0, degrees, rounds)
        assert 0 < (~ok).sum() < N
        rot, centre = pa.ORACLE_WORST[0, degrees, rounds]
        assert rot <= pa.BOUND_ROT_DEG and centre <= pa.BOUND_CENTRE_M
        assert last["rot_err"][ok].max() <= rot and last["centre_err"][ok].max() <= centre
        assert (last["rmse"][ok] < last["rmse_initial"][ok]).all() or rounds > 1


def test_the_spread_falls():
    """the fusion's mean spread at the returned cameras (depth images re-rendered there) is below the spread at the start, both sizes"""
    for size in range(len(cc.SIZES)):
        last, ok = check_alignment(size, 0.5, 1)
        R0, t0, d0 = last["start"]
        before = pa.spread(size, R0, t0, d0)
        after = pa.spread(size, last["Rcw"], last["tcw"], pa.rerendered(size, last["Rcw"], last["tcw"]))
        truth = pa.spread(size, *pa.poses(size, "planted"))
        print(f"size {cc.SIZES[size]}: mean spread {before:.3f} -> {after:.3f} (planted cameras: {truth:.3f})")
        assert after < before


def test_header_iteration_equals_the_oracles(emul):
    """pal_step driven on the host against align_image: the same statuses, passes and accepted steps on the cameras of the fixture
    (the sums differ in their last bits: a walk here, pairwise there), the poses to 1e-9; refused poses bit for bit"""
    s = pc.scene(0)
    ref16, valid = pa.reference(0)
    r = pa.aligned(0, 0.5, 1)[0]
    R, t, depth = r["start"]
    for j in range(N):
        g = host_align(emul, s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j])
        assert g["status"] == r["status"][j] and int(g["cur"][pao.CNT]) == r["n_samples"][j], j
        if g["status"] == pao.TOO_FEW_SAMPLES:
            assert same_bytes(g["Rcw"], R[j]) and same_bytes(g["tcw"], t[j]) and g["iterations"] == 1
        else:
            assert np.abs(g["Rcw"] - r["Rcw"][j]).max() <= 1e-9 and np.abs(g["tcw"] - r["tcw"][j]).max() <= 1e-9, j
    # the other states, on one camera: out of bounds below the planted turn, degenerate on a constant image, one pass only
    j = 0
    g = host_align(emul, s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j], max_rotation_deg=0.1)
    e = pao.align_image(s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j], max_rotation_deg=0.1)
    assert g["status"] == e["status"] == pao.OUT_OF_BOUNDS and same_bytes(g["Rcw"], R[j]) and same_bytes(g["tcw"], t[j])
    assert same_bytes(g["cur"], g["first"])
    flat = pc.constant_images(0)[0][j]
    g = host_align(emul, s["points"], ref16, valid, flat, depth[j], s["intr"], R[j], t[j])
    e = pao.align_image(s["points"], ref16, valid, flat, depth[j], s["intr"], R[j], t[j])
    assert g["status"] == e["status"] == pao.DEGENERATE and same_bytes(g["Rcw"], R[j]) and g["iterations"] == 1
    assert not g["cur"][:27].any()                                               # every gradient is 0: H = 0, g = 0
    g = host_align(emul, s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j], max_iterations=1)
    assert g["status"] == pao.MAX_ITERATIONS and g["iterations"] == 1 and same_bytes(g["Rcw"], R[j])
    # CONVERGED, with thresholds the iteration reaches within its passes: every camera, against the oracle's loop
    loose = dict(eps_rot=1e-3, eps_trans=1e-2)
    e = pa.aligned(0, 0.5, 1, **loose)[0]
    for size in range(len(cc.SIZES)):                                          # the fixture's conditions at the poses these runs visit
        q = pa.aligned(size, 0.5, 1, **loose)[0]
        assert q["margins"]["compare"] >= mc.MIN_MARGIN and q["margins"]["texel"] >= pc.TEXEL_MARGIN and q["min_gap"] >= pa.MIN_GAP
    assert (e["status"] == pao.CONVERGED).sum() >= 10
    for j in range(N):
        g = host_align(emul, s["points"], ref16, valid, s["images"][j], depth[j], s["intr"], R[j], t[j], **loose)
        assert (g["status"], g["iterations"], g["accepted"]) == (e["status"][j], e["iterations"][j], e["accepted"][j]), j
        assert np.abs(g["Rcw"] - e["Rcw"][j]).max() <= 1e-9 and np.abs(g["tcw"] - e["tcw"][j]).max() <= 1e-9, j
        if g["status"] == pao.CONVERGED:
            assert 1 < g["iterations"] < pao.DEFAULTS["max_iterations"] and g["accepted"] >= 1
            assert not same_bytes(g["Rcw"], R[j]) and g["cur"][pao.SSQ] < g["first"][pao.SSQ]       # the accepted pose is what comes back


# ------------------------------------------------------------------------------------------------------------- 5. the binding
def test_struct_sizes_defaults_and_the_reference_helper(pkg):
    L = pkg._lib
    assert ctypes.sizeof(L.PalignOpts) == 88
    import __graft_entry__ as ge
    ge.build()
    PA = importlib.import_module("global-lvba_amd.palign")
    o = PA.palign_opts()
    assert {k: getattr(o, k) for k in PA.OPTION_NAMES} == pao.DEFAULTS
    assert list(PA.OPTION_NAMES) == list(pao.DEFAULTS)
    with pytest.raises(TypeError, match="photometric alignment"):
        PA.palign_opts(no_such=1)
    assert PA.PhotoAligner._destroy == "lvba_palign_free" and PA.PhotoAligner._destroy in L.SYMBOLS
    assert (PA.CONVERGED, PA.MAX_ITERATIONS, PA.TOO_FEW_SAMPLES, PA.DEGENERATE, PA.OUT_OF_BOUNDS) == \
        (pao.CONVERGED, pao.MAX_ITERATIONS, pao.TOO_FEW_SAMPLES, pao.DEGENERATE, pao.OUT_OF_BOUNDS)
    e = pc.expected(1)
    for mv in (1, 2, 3):
        ref, ok = PA.reference_from_sums(e["n_views"], e["s1"], mv)
        wr, wo = pao.reference_from_sums(e["n_views"], e["s1"], mv)
        assert same_bytes(ref, wr) and same_bytes(ok, wo) and ok.sum() == (e["n_views"] >= mv).sum()
    k = int(np.flatnonzero(e["n_views"] >= 3)[0])
    n, s1 = int(e["n_views"][k]), [int(x) for x in e["s1"][k]]
    assert PA.reference_from_sums(e["n_views"], e["s1"])[0][k].tolist() == [(2 * x + n) // (2 * n) for x in s1]
    u = PA.unpack_sums(np.arange(31.0)[None])
    assert u["H"][0, 0, 5] == u["H"][0, 5, 0] == 5 and u["H"][0, 5, 5] == 20 and u["g"][0].tolist() == list(range(21, 27))
    assert (u["cost"][0], u["n_samples"][0], u["sum_sq"][0], u["sum_w"][0]) == (27, 28, 29, 30)


def test_the_ramp_case_in_exact_arithmetic_on_the_host(emul):
    """palign_cases.ramp_case: the header's sums equal the closed form, not a bit apart (the GPU test asks the same of the device)"""
    c = pa.ramp_case()
    g = host_records(emul, c["points"], c["ref16"], c["valid"], c["image"][0], None, c["intr"], np.eye(3), np.zeros(3), loss_kind=0)
    np.testing.assert_array_equal(g["seen"].astype(bool), c["inside"])
    i = np.flatnonzero(c["inside"])
    assert (g["gu"][i] == [1.0, 0.0, 1.0]).all() and (g["gv"][i] == [0.0, 1.0, 1.0]).all() and (g["r"][i] == [-0.5, -0.25, -1.0]).all()
    assert same_bytes(pao.expand(g["sums"]), c["Hm"]) and same_bytes(g["sums"][pao.G0:pao.G0 + 6], c["g"])
    assert g["sums"][pao.COST] == c["cost"] and g["sums"][pao.SSQ] == c["sum_sq"] and g["sums"][pao.CNT] == c["n_samples"] == 81
    assert g["sums"][pao.SW] == 3 * c["n_samples"]


# ------------------------------------------------------------------------------------------------------------ 6. the pipeline
class _FakeScans:
    device = 0

    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


class _FakeDepth(_FakeScans):
    rendered = []

    @classmethod
    def render(cls, scans, poses, scan_times, image_times, Rcw, tcw, *a, **k):
        cls.rendered.append((Rcw, tcw))
        return cls()


ARGS = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
        np.ones(8), 640, 512, [np.zeros((5, 2), np.float32)] * 2, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])


def _fake_pipeline(monkeypatch, pl):
    visual = dict(Rcw=np.ones((2, 3, 3)), tcw=np.ones((2, 3)), Rcw_before=np.zeros((2, 3, 3)), tcw_before=np.zeros((2, 3)))
    after, before = (np.ones((4, 3), np.float32), np.zeros((4, 3), np.uint8)), (np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: dict(visual))
    monkeypatch.setattr(pl, "colorize_maps", lambda *a, **k: dict(after=after, before=before))
    return visual, after, before


def test_the_default_path_calls_no_palign_entry_point(monkeypatch):
    """photo_align=None (the default) neither imports the palign module nor asks the loaded library for an lvba_palign_* entry point, with and without
    images; and the keyword without images is refused"""
    import sys
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")

    class NoPalignLib:
        def __getattr__(self, name):
            if name.startswith("lvba_palign"):
                pytest.fail(f"{name} looked up on the default path")
            raise AttributeError(name)

    _fake_pipeline(monkeypatch, pl)
    monkeypatch.setattr(pl, "_align_cameras_photometric", lambda *a, **k: pytest.fail("the stage ran on the default path"))
    monkeypatch.setattr(L, "load", lambda: NoPalignLib())
    sys.modules.pop("global-lvba_amd.palign", None)
    for kw in (dict(), dict(images=np.zeros((2, 512, 640, 3), np.uint8)), dict(photo_align=None), dict(photo_align=False)):
        out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, **kw)
        assert not [k for k in out if k.startswith("photo_align")]
    assert "global-lvba_amd.palign" not in sys.modules
    with pytest.raises(ValueError, match="images"):
        pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, photo_align=True)


def test_run_full_pipeline_hands_the_cameras_on(monkeypatch):
    """the alignment gets colored_after's points, the refined cameras and depth images rendered at them; True reports only,
    "apply" hands the aligned cameras to the `after` set of the photometric consistency and to nothing else"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    visual, after, before = _fake_pipeline(monkeypatch, pl)
    monkeypatch.setattr(pl.V, "DepthImages", _FakeDepth)
    aligned = (np.full((2, 3, 3), 7.0), np.full((2, 3), 7.0))
    calls, fused = [], []

    def fake_align(points, images, cameras, depth, intr, width, height, **kw):
        calls.append((points, cameras, depth, kw))
        return dict(Rcw=aligned[0], tcw=aligned[1], status=np.zeros(2, np.int32), status_names=["CONVERGED"] * 2, information=np.zeros((2, 6, 6)),
                    rmse_initial=np.ones(2), rmse=np.zeros(2), mean_sigma=[2.0, 1.0], rounds=[], options={})

    def fake_fuse(scans, scan_times, image_times, images, intr, width, height, after, before, points_after, points_before, **kw):
        fused.append((after, before))
        one = lambda p: dict(summary=dict(n_points=len(p)), n_views=np.zeros(len(p), np.int32), rgb=np.zeros((len(p), 3), np.uint8),
                             sigma=np.zeros(len(p)), options={})
        return dict(after=one(points_after), before=one(points_before))

    monkeypatch.setattr(pl, "_align_cameras_photometric", fake_align)
    monkeypatch.setattr(pl, "_photo_consistency", fake_fuse)
    images = np.zeros((2, 512, 640, 3), np.uint8)
    for mode, applied in ((True, False), ("apply", True), (dict(rounds=2, min_samples=50), False), (dict(apply=True, rounds=3), True)):
        calls.clear(); fused.clear(); _FakeDepth.rendered.clear()
        out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=images, photo_align=mode, photo_consistency=True)
        (points, cameras, depth, kw), = calls
        assert points is after[0] and cameras[0] is visual["Rcw"] and cameras[1] is visual["tcw"] and isinstance(depth, _FakeDepth)
        assert _FakeDepth.rendered[0][0] is visual["Rcw"] and callable(kw.pop("render")) and kw.pop("device") == 0
        assert kw == ({k: v for k, v in mode.items() if k != "apply"} if isinstance(mode, dict) else {})
        assert out["photo_align"]["applied"] is applied and "information" not in out["photo_align"] and "Rcw" not in out["photo_align"]
        assert out["photo_align_cameras"][0] is aligned[0] and out["photo_align"]["mean_sigma"] == [2.0, 1.0]
        (a, b), = fused
        assert (a[1] is aligned[0] and a[2] is aligned[1]) if applied else (a[1] is visual["Rcw"] and a[2] is visual["tcw"])
        assert b[1] is visual["Rcw_before"] and out["colored_after"] is after and out["visual"]["Rcw"] is visual["Rcw"]
    out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=images, photo_align=True)           # without the consistency stage
    assert "photo_align" in out and "fused_after" not in out


def test_run_dataset_hands_the_keyword_on_and_writes_the_report(tmp_path, monkeypatch):
    import json
    import sqlite3
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    for t in (0.5, 1.5):
        ds.save_pcd(str(tmp_path / "all_pcd_body" / f"{t}.pcd"), rng.normal(size=(10, 4)).astype(np.float32))
        (tmp_path / "all_image" / f"{t}.png").write_bytes(b"")
    (tmp_path / "all_pcd_body" / "lidar_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    (tmp_path / "all_image" / "image_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    con = sqlite3.connect(str(tmp_path / "db.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    kp = rng.uniform(0, 500, (6, 4)).astype(np.float32)
    for iid, name in ((1, "0.500000.png"), (2, "1.500000.png")):
        con.execute("INSERT INTO images VALUES (?, ?)", (iid, name))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (iid, 6, 4, kp.tobytes()))
    con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                (ds.image_ids_to_pair_id(1, 2), 2, 2, np.array([[0, 1], [2, 3]], np.uint32).tobytes()))
    con.commit(); con.close()
    report = dict(status=np.array([0, 2], np.int32), status_names=["CONVERGED", "TOO_FEW_SAMPLES"], rmse_initial=np.array([3.0, 1.0]),
                  rmse=np.array([0.25, 1.0]), mean_sigma=[2.0, 1.5], rounds=[dict(status=np.array([0, 2], np.int32), n_valid=4)],
                  options=dict(pao.DEFAULTS), applied=False)
    calls = []

    def full_pipeline(*a, **k):
        calls.append(k)
        extra = dict(photo_align=report, photo_align_cameras=(np.zeros((2, 3, 3)), np.zeros((2, 3)))) if k.get("photo_align") else {}
        return dict(extra, poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1)))

    monkeypatch.setattr(pl, "run_full_pipeline", full_pipeline)
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir))
    assert "photo_align" not in calls[0] and calls[0]["images"] is None and not (out_dir / "photo_align.json").exists()
    pl.run_dataset(*args, out_dir=str(out_dir), photo_align=dict(rounds=2))
    assert calls[1]["photo_align"] == dict(rounds=2) and callable(calls[1]["images"])          # the images are read without colorize=True
    rep = json.load(open(out_dir / "photo_align.json"))
    assert rep["status"] == [0, 2] and rep["status_names"] == report["status_names"] and rep["rmse"] == [0.25, 1.0]
    assert rep["mean_sigma"] == [2.0, 1.5] and rep["rounds"] == [dict(status=[0, 2], n_valid=4)] and rep["options"] == pao.DEFAULTS
    assert rep["applied"] is False
