"""CPU tests of the camera resectioning's rule and fixtures (include/lvba_hip.h "camera resectioning from 2-D to 3-D matches",
DESIGN.md §10n): csrc/resect_device.h on the host against the numpy oracle to the bit, the sampler, the minimal solver on
noise-free samples, the refits and the information matrix under measured tolerances, the margin condition of the fixtures, what
the fixtures claim, and the default paths of run_full_pipeline and run_dataset."""
import ctypes
import importlib
import sys

import numpy as np
import pytest

import resect_cases as rc
import resect_oracle as ro
import verify_oracle as vo
from host_build import build_check

# The largest difference between the pose after the host emulation's refinement rounds (4 Gauss-Newton steps a round, Cholesky,
# quaternion) and the oracle's (the same residual minimised to convergence with lstsq) over all fixtures that reach the refinement
# with at least 30 inliers, measured on the CPU (test_refits_agree_within_the_measured_tolerance prints both): Frobenius norm of
# the rotations' difference 1.07e-15, and |t - t'| / |t'| 1.07e-12.  The tests allow ten times that: the device sums in another order.
REFIT_D_R = 1.1e-15
REFIT_D_T = 1.1e-12
REFIT_TOL_R, REFIT_TOL_T = 10 * REFIT_D_R, 10 * REFIT_D_T
# What the order of summation alone changes in a refined pose: the largest difference between the host emulation's refinement with
# its sums taken first to last and the same with them taken last to first or as 256 strided partial sums, over EVERY fixture with a
# winner, jobs of three inliers included (58 jobs; the same test prints it): 2.5e-16 and 8.5e-13.  The device's sums are a fourth
# order; every pose it refines is held to ten times this against the host emulation (tests/test_gpu_resect.py).
ORDER_D_R = 2.5e-16
ORDER_D_T = 8.5e-13
ORDER_TOL_R, ORDER_TOL_T = 10 * ORDER_D_R, 10 * ORDER_D_T
# The largest pose error of the minimal solver on noise-free samples over all scenes (test_p3p_on_noise_free_samples prints it):
# Frobenius norm for R, |t - t'| for t (metres; |t| is 0 for view 0), and the relative residual of the three distance equations.
# The worst samples are thin triangles; the assertion allows ten times these.
P3P_D_R, P3P_D_T, P3P_D_EQ = 8.4e-8, 4.2e-7, 1.1e-9
# information against central finite differences of the oracle's residual: step 1e-6 (radians, metres); the largest relative
# difference |I - I_fd| / max|I| measured over the claims is INFO_D; the test allows ten times that.
INFO_STEP = 1e-6
INFO_D = 3.5e-11


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/resect_device.h compiled for the host, without contraction (tests/resect_check.cpp)"""
    lib = ctypes.CDLL(build_check("resect_check", tmp_path_factory.mktemp("emul_resect")))
    P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    lib.emul_pack.argtypes = [I, P, P, P]
    lib.emul_pack.restype = None
    lib.emul_sample.argtypes = [ctypes.c_uint64, I, I, I, P]
    lib.emul_sample.restype = None
    lib.emul_p3p.argtypes = [P, D, D, P, P]
    lib.emul_score.argtypes = [I, P, P, P, D, D, D, P]
    lib.emul_score.restype = None
    lib.emul_hypotheses.argtypes = [ctypes.c_uint64, I, I, I, P, D, D, D, P, P, P]
    lib.emul_refine.argtypes = [I, P, D, D, D, I, I, I, P, P, P, P]
    lib.emul_orthonormalise.argtypes = [P]
    lib.emul_orthonormalise.restype = None
    lib.emul_status.argtypes = [I, I, I]
    return lib


def host_hypotheses(emul, case, **over):
    o = rc.options(case, **over)
    rec = np.ascontiguousarray(case["rec"])
    intr = case["scene"]["intr"]
    H = o["hypotheses"]
    R, t, count = np.zeros((H, 9)), np.zeros((H, 3)), np.full(H, -1, np.int32)
    win = -1
    if len(rec) >= ro.K:
        win = emul.emul_hypotheses(o["seed"], case["id"], H, len(rec), rec.ctypes.data, intr[0], intr[1], o["max_error_px"], R.ctypes.data,
                                   t.ctypes.data, count.ctypes.data)
    return R, t, count, win


def host_refine(emul, case, R, t, count, rounds=2, order=0, **over):
    o = rc.options(case, **over)
    rec = np.ascontiguousarray(case["rec"])
    intr = case["scene"]["intr"]
    R, t = np.ascontiguousarray(R, np.float64).copy(), np.ascontiguousarray(t, np.float64).copy()
    info, rmse = np.zeros(36), ctypes.c_double()
    c = emul.emul_refine(len(rec), rec.ctypes.data, intr[0], intr[1], o["max_error_px"], rounds, int(count), int(order), R.ctypes.data,
                         t.ctypes.data, info.ctypes.data, ctypes.addressof(rmse))
    return R, t, c, info.reshape(6, 6), rmse.value


def test_sampler_is_distinct_in_range_and_counter_based(emul):
    for m in (4, 5, 10 ** 4):
        got = np.zeros((300, 4), np.int32)
        emul.emul_sample(5, 17, 300, m, got.ctypes.data)
        np.testing.assert_array_equal(got, ro.sample(5, 17, 300, m))
        assert got.min() >= 0 and got.max() < m
        assert all(len(set(r.tolist())) == 4 for r in got)
    full = ro.sample(9, 3, 200, 500)
    np.testing.assert_array_equal(ro.sample(9, 3, 77, 500), full[:77])           # a hypothesis alone draws what it draws in a longer run
    for other in ((10, 3), (9, 4)):
        assert (ro.sample(*other, 200, 500) != full).any()
    for lo, hi in ((3, 4), (0, 3), (3, 0xFFFFFFFE)):                             # apart from every image pair's stream
        assert (vo.sample(9, lo, hi, 200, 500, 4) != full).any()
    hist = np.bincount(ro.sample(3, 0, 4000, 50).ravel(), minlength=50)
    assert hist.min() > 0.7 * hist.mean() and hist.max() < 1.3 * hist.mean()


def test_device_header_on_the_host_equals_the_oracle(emul):
    """Every hypothesis's R, t and count, the winner and the masks of every fixture the GPU tests use, bit for bit: the solver uses
    +, -, *, / and sqrt only, in one order."""
    seen, worst = 0, np.inf
    for case in rc.all_gpu_cases():
        R, t, count, idx, margin = rc.oracle_hypotheses(case)
        worst = min(worst, margin)
        gR, gt, gcount, win = host_hypotheses(emul, case)
        np.testing.assert_array_equal(gR, R, err_msg=case["name"])
        np.testing.assert_array_equal(gt, t, err_msg=case["name"])
        np.testing.assert_array_equal(gcount, count, err_msg=case["name"])
        assert win == ro.pick(count)[0], case["name"]
        seen += int((count >= 0).sum())
        if win >= 0:
            rec = np.ascontiguousarray(case["rec"])
            intr = case["scene"]["intr"]
            mask = np.zeros(len(rec), np.uint8)
            emul.emul_score(len(rec), rec.ctypes.data, np.ascontiguousarray(R[win]).ctypes.data, np.ascontiguousarray(t[win]).ctypes.data,
                            intr[0], intr[1], 8.0, mask.ctypes.data)
            np.testing.assert_array_equal(mask.astype(bool), ro.score(R[win], t[win], rec, intr, 8.0))
            assert mask.sum() == count[win]
    assert seen > 10000
    # the margin condition that lets the comparison be exact on the device too: no inlier decision and no solver threshold
    # (resect_oracle.p3p lists them) of any fixture within 1e-9 relative of its bound, nothing excluded
    print("smallest relative margin of any (fixture, hypothesis, correspondence or threshold):", worst)
    assert worst >= rc.MIN_MARGIN, worst
    # the record: undistortion and the marking of unusable correspondences
    case = rc.general()["claims"][1]
    xy = ro.mo.undistort_all(case["scene"]["intr"], case["uv"])
    rec = np.zeros((len(xy), 5))
    emul.emul_pack(len(xy), np.ascontiguousarray(xy).ctypes.data, np.ascontiguousarray(case["world"]).ctypes.data, rec.ctypes.data)
    np.testing.assert_array_equal(rec, case["rec"])
    assert np.isnan(rec[:, 0]).sum() == 5                                       # three keypoints and two world points
    for m, mi, c, want in ((3, 0, -1, ro.TOO_FEW_MATCHES), (29, 30, 29, ro.TOO_FEW_MATCHES), (40, 30, -1, ro.NO_MODEL),
                           (40, 30, 29, ro.TOO_FEW_INLIERS), (40, 30, 30, ro.OK), (4, 0, 0, ro.OK)):
        assert emul.emul_status(m, mi, c) == want


def test_p3p_on_noise_free_samples(emul):
    """Exact projections: the solution the fourth point picks maps the three points onto their bearings at the depths that satisfy
    the three distance equations, and is the true pose."""
    worst_R = worst_t = worst_eq = 0.0
    n = 0
    for fx_ in (rc.general(), rc.planar()):
        sc = fx_["scene"]
        rng = np.random.default_rng(5)
        for view in range(4):
            Rw, tw = sc["Rcw"][view], sc["tcw"][view]
            for _ in range(200):
                X = sc["X"][rng.choice(len(sc["X"]), 4, replace=False)]
                Xc = X @ Rw.T + tw
                c = np.ascontiguousarray(np.concatenate([Xc[:, :2] / Xc[:, 2:3], X], 1))
                R, t = np.zeros(9), np.zeros(3)
                if not emul.emul_p3p(c.ctypes.data, sc["intr"][0], sc["intr"][1], R.ctypes.data, t.ctypes.data):
                    continue
                n += 1
                Y = X[:3] @ R.reshape(3, 3).T + t
                s = np.linalg.norm(Y, axis=1)
                f = np.concatenate([c[:3, :2], np.ones((3, 1))], 1)
                f /= np.linalg.norm(f, axis=1, keepdims=True)
                for i, j in ((0, 1), (0, 2), (1, 2)):
                    a = ((X[i] - X[j]) ** 2).sum()
                    worst_eq = max(worst_eq, abs(s[i] ** 2 + s[j] ** 2 - 2 * s[i] * s[j] * (f[i] @ f[j]) - a) / a)
                worst_R = max(worst_R, np.linalg.norm(R - Rw.reshape(9)))
                worst_t = max(worst_t, np.linalg.norm(t - tw))
    print("noise-free P3P over", n, "samples: largest |R - R*|_F", worst_R, " |t - t*|", worst_t, " distance equations (relative)", worst_eq)
    assert n > 1500
    assert worst_R <= 10 * P3P_D_R and worst_t <= 10 * P3P_D_T and worst_eq <= 10 * P3P_D_EQ


def host_job(emul, case, **over):
    """the whole job through the host build of the device header: dict(R, t, R0, t0, count0, n_inliers, best_h, status, mask)"""
    o = rc.options(case, **over)
    rec, intr = np.ascontiguousarray(case["rec"]), case["scene"]["intr"]
    out = dict(R=np.zeros(9), t=np.zeros(3), R0=np.zeros(9), t0=np.zeros(3), count0=0, n_inliers=0, best_h=-1, mask=np.zeros(len(rec), bool),
               status=emul.emul_status(len(rec), o["min_inliers"], -1))
    if out["status"] == ro.TOO_FEW_MATCHES:
        return out
    R, t, count, win = host_hypotheses(emul, case, **over)
    if win < 0:
        return out
    fR, ft, c, _, _ = host_refine(emul, case, R[win], t[win], count[win], rounds=o["refine_rounds"], **over)
    out.update(R=fR, t=ft, R0=R[win], t0=t[win], count0=int(count[win]), n_inliers=c, best_h=win, status=emul.emul_status(len(rec), o["min_inliers"], c))
    if out["status"] == ro.OK:
        out["mask"] = host_score(emul, rec, intr, fR, ft, o["max_error_px"])
    return out


def host_score(emul, rec, intr, R, t, rho):
    mask = np.zeros(len(rec), np.uint8)
    emul.emul_score(len(rec), np.ascontiguousarray(rec).ctypes.data, np.ascontiguousarray(R, np.float64).ctypes.data,
                    np.ascontiguousarray(t, np.float64).ctypes.data, intr[0], intr[1], float(rho), mask.ctypes.data)
    return mask.astype(bool)


def test_outliers_are_off_their_images(emul):
    """under the true pose the header's own test takes in no planted outlier at 20 px and every planted inlier at 2.5 px"""
    for fx_ in (rc.general(), rc.planar()):
        for case in fx_["claims"]:
            R, t = rc.truth(case)
            intr = case["scene"]["intr"]
            r = np.linalg.norm(ro.residuals(R, t, case["rec"], intr), axis=1)
            out = ~case["planted"] & np.isfinite(r)
            assert out.sum() > 30 and r[out].min() >= rc.OUTLIER_PX
            assert r[case["planted"]].max() < 2.5                               # 0.3 px of noise
            assert not host_score(emul, case["rec"], intr, R, t, rc.OUTLIER_PX)[~case["planted"]].any()
            assert host_score(emul, case["rec"], intr, R, t, 2.5)[case["planted"]].all()


def test_fixture_claims(emul):
    """What the fixtures claim, of the oracle and of the host build of the device header alike."""
    g, p = rc.general(), rc.planar()
    # 40 % outliers in general position and 60 % on the single plane: exactly the planted set, also with unusable correspondences
    for case in g["claims"] + p["claims"]:
        for r in (rc.oracle_job(case), host_job(emul, case)):
            assert r["status"] == ro.OK
            np.testing.assert_array_equal(r["mask"], case["planted"], err_msg=case["name"])
    # on EVERY fixture that comes back OK the refined pose is nearer the truth than the winning hypothesis, in rotation and in
    # translation (resect_cases.GENERAL_SEED is chosen so that this holds; nothing is excluded)
    n_ok = 0
    for case in rc.all_gpu_cases():
        want, got = rc.oracle_job(case), host_job(emul, case)
        assert got["status"] == want["status"] and got["best_h"] == want["best_h"], case["name"]
        if want["status"] != ro.OK:
            continue
        n_ok += 1
        Rt, tt = rc.truth(case)
        for who, r in (("oracle", want), ("host", got)):
            a1, d1 = ro.pose_offset(r["R"], r["t"], Rt, tt)
            a0, d0 = ro.pose_offset(r["R0"], r["t0"], Rt, tt)
            if who == "oracle":
                print(case["name"], "hypothesis: %.4f deg %.4f m;  refined: %.4f deg %.4f m;  rmse %.3f px" % (a0, d0, a1, d1, r["rmse_px"]))
            assert a1 < a0 and d1 < d0, (case["name"], who)
    assert n_ok >= 40
    # an unusable correspondence is never an inlier, and a sample that holds one is invalid
    case = g["claims"][1]
    rec = case["rec"]
    bad = np.isnan(rec[:, 0])
    R, t, count, idx, _ = rc.oracle_hypotheses(case)
    hcount = host_hypotheses(emul, case)[2]
    assert bad.sum() == 5 and (hcount[bad[idx].any(axis=1)] == -1).all() and bad[idx].any(axis=1).sum() > 0
    Rt, tt = rc.truth(case)
    assert not host_score(emul, rec, case["scene"]["intr"], Rt, tt, 8.0)[bad].any()
    behind = (case["world"] @ Rt.reshape(3, 3).T + tt)[:, 2] < 0
    assert behind.sum() == 2 and not host_score(emul, rec, case["scene"]["intr"], Rt, tt, 8.0)[behind].any()
    # one correspondence repeated: no model
    for case in g["special"]:
        for r in (rc.oracle_job(case), host_job(emul, case)):
            assert r["status"] == ro.NO_MODEL and r["best_h"] == -1 and not r["R"].any() and not r["mask"].any()
    # the same job under two ids draws other samples and finds the same inliers
    r0, r1 = (host_job(emul, c) for c in g["two_ids"])
    assert (rc.oracle_hypotheses(g["two_ids"][0])[3] != rc.oracle_hypotheses(g["two_ids"][1])[3]).any()
    np.testing.assert_array_equal(r0["mask"], r1["mask"])
    # the statuses of the size ladder
    for case in g["sizes"]:
        for job in (lambda **k: rc.oracle_job(case, **k), lambda **k: host_job(emul, case, **k)):
            assert (job()["status"] == ro.TOO_FEW_MATCHES) == (len(case["rec"]) < 30), case["name"]
            assert (job(min_inliers=0)["status"] == ro.TOO_FEW_MATCHES) == (len(case["rec"]) < 4), case["name"]


def test_refits_agree_within_the_measured_tolerance(emul):
    """The host emulation's refinement rounds against the oracle's converged fits from the same winner; and, on every job with a
    winner, against themselves with the sums taken in two other orders (tests/resect_check.cpp) -- what the order of summation
    alone changes."""
    dR = dt = oR = ot = 0.0
    n, n_all, worst, worst_o = 0, 0, None, None
    for case in rc.all_gpu_cases():
        r = rc.oracle_job(case, min_inliers=0)
        if r["best_h"] < 0:
            continue
        R, t, c, info, rmse = host_refine(emul, case, r["R0"], r["t0"], r["count0"])
        assert c >= r["count0"], case["name"]
        for order in (1, 2):
            R2, t2, c2, _, _ = host_refine(emul, case, r["R0"], r["t0"], r["count0"], order=order)
            assert c2 == c, case["name"]
            a, b = ro.pose_difference(R2, t2, R, t)
            if a > oR or b > ot:
                worst_o = (case["name"], len(case["rec"]), c)
            oR, ot = max(oR, a), max(ot, b)
        n_all += 1
        if r["count0"] < 30:                     # a fit over a handful of inliers is as good as its conditioning: held to ORDER_D only
            continue
        assert c == r["n_inliers"], case["name"]
        np.testing.assert_array_equal(ro.score(R, t, case["rec"], case["scene"]["intr"], 8.0),
                                      ro.score(r["R"], r["t"], case["rec"], case["scene"]["intr"], 8.0))
        assert abs(np.linalg.det(R.reshape(3, 3)) - 1.0) < 1e-14 and np.abs(R.reshape(3, 3) @ R.reshape(3, 3).T - np.eye(3)).max() < 1e-14
        a, b = ro.pose_difference(R, t, r["R"], r["t"])
        if a > dR or b > dt:
            worst = case["name"]
        dR, dt = max(dR, a), max(dt, b)
        assert abs(rmse - r["rmse_px"]) < 1e-9
        n += 1
    print("largest refit difference over", n, "jobs: |R - R'|_F", dR, " |t - t'| / |t'|", dt, "in", worst)
    print("largest difference between the orders of summation over", n_all, "jobs: |R - R'|_F", oR, " |t - t'| / |t'|", ot, "in", worst_o)
    assert n > 30 and dR <= REFIT_TOL_R and dt <= REFIT_TOL_T
    assert n_all > n and oR <= ORDER_TOL_R and ot <= ORDER_TOL_T


def test_orthonormalise_takes_every_branch(emul):
    """R -> unit quaternion -> R on rotations near the identity (the trace leads) and by 170 - 180 degrees about each axis and
    about a diagonal (each diagonal entry leads in turn): a rotation comes back to rounding, a perturbed one comes back
    orthonormal and no further from the input than the perturbation."""
    rng = np.random.default_rng(3)
    lead = set()
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, -2, 0.5], [0.3, 0.2, -2]):
        for ang in (0.03, 1.0, 2.97, np.pi - 1e-9, np.pi):
            w = np.asarray(axis, np.float64) / np.linalg.norm(axis) * ang
            R0 = ro.rodrigues(w)
            lead.add(int(np.argmax([np.trace(R0), R0[0, 0], R0[1, 1], R0[2, 2]])))
            R = np.ascontiguousarray(R0.reshape(9).copy())
            emul.emul_orthonormalise(R.ctypes.data)
            assert np.abs(R - R0.reshape(9)).max() < 1e-15 * 8, (axis, ang)
            E = 1e-6 * rng.standard_normal(9)
            R = np.ascontiguousarray(R0.reshape(9) + E)
            emul.emul_orthonormalise(R.ctypes.data)
            Q = R.reshape(3, 3)
            assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-15 * 8 and abs(np.linalg.det(Q) - 1.0) < 1e-14
            assert np.linalg.norm(R - R0.reshape(9)) <= 2.0 * np.linalg.norm(E)
    assert lead == {0, 1, 2, 3}


def test_information_against_finite_differences(emul):
    d = 0.0
    for case in rc.general()["claims"] + rc.planar()["claims"]:
        r = rc.oracle_job(case)
        R, t, c, info, _ = host_refine(emul, case, r["R"], r["t"], r["n_inliers"], rounds=0)
        np.testing.assert_array_equal(R, r["R"])
        inl = case["rec"][ro.score(R, t, case["rec"], case["scene"]["intr"], 8.0)]
        fd = ro.information_fd(R, t, inl, case["scene"]["intr"], INFO_STEP)
        d = max(d, float(np.abs(info - fd).max() / np.abs(fd).max()))
        assert np.abs(info - info.T).max() == 0.0 and np.linalg.eigvalsh(info).min() > 0
    print("largest relative difference between information and its finite-difference form:", d)
    assert d <= 10 * INFO_D


class _FakeScans:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


def test_run_full_pipeline_without_the_check_is_the_untouched_path(monkeypatch):
    """check_cameras=None (the default) hands the visual stage exactly what the call without the keyword hands it, and neither
    imports the resect module nor looks a new entry point up."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")

    class NoResectLib:
        """a library that fails the test when a resect entry point is looked up"""
        def __getattr__(self, name):
            if name.startswith("lvba_resect"):
                pytest.fail(f"{name} looked up on the default path")
            raise AttributeError(name)

    calls = []
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(pl, "_check_cameras", lambda *a, **k: pytest.fail("the camera check ran on the default path"))
    monkeypatch.setattr(L, "load", lambda: NoResectLib())
    sys.modules.pop("global-lvba_amd.resect", None)
    kps = [np.zeros((5, 2), np.float32)] * 2
    args = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
            np.ones(8), 640, 512, kps, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])
    out0 = pl.run_full_pipeline(*args, enable_lidar_ba=False)
    out1 = pl.run_full_pipeline(*args, enable_lidar_ba=False, check_cameras=None)
    assert "global-lvba_amd.resect" not in sys.modules
    (a0, k0), (a1, k1) = calls
    assert k0.keys() == k1.keys() and len(a0) == len(a1)
    for x, y in zip(a0[1:], a1[1:]):
        assert repr(x) == repr(y)
    assert "camera_check" not in out0 and "camera_check" not in out1


def test_correspondences_from_matches_uses_both_directions_in_order():
    pl = importlib.import_module("global-lvba_amd.pipeline")
    nan = np.nan
    points = [np.array([[1., 0, 0], [nan, nan, nan], [3, 0, 0]]), np.array([[10., 0, 0], [11, 0, 0]]), np.array([[nan, nan, nan]])]
    pairs = [(1, 0), (0, 2)]
    matches = [np.array([[0, 2], [1, 1], [1, 0]]), np.array([[2, 0]])]
    kp, X = pl.correspondences_from_matches(pairs, matches, points)
    np.testing.assert_array_equal(kp[0], [2, 1, 0])              # image 0 is the second image of pair (1, 0); pair (0, 2) gives it nothing
    np.testing.assert_array_equal(X[0], [[10, 0, 0], [11, 0, 0], [11, 0, 0]])
    np.testing.assert_array_equal(kp[1], [0, 1])                 # the match onto keypoint 1 of image 0 has no point
    np.testing.assert_array_equal(X[1], [[3, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(kp[2], [0])
    np.testing.assert_array_equal(X[2], [[3, 0, 0]])
    assert kp[0].dtype == np.int32 and X[2].shape == (1, 3)


def test_run_dataset_hands_check_cameras_on_and_writes_the_report(tmp_path, monkeypatch):
    """run_dataset(check_cameras=...) passes the keyword to run_full_pipeline, writes camera_check.json, and without the keyword
    passes nothing."""
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
    calls = []
    report = dict(images=[dict(image=0, status="too_few_matches", n_matches=2, n_inliers=0, rmse_px=0.0)], n_images=1, n_images_ok=0,
                  median_rotation_deg=None, median_translation=None, poses=[[0.0] * 12])
    monkeypatch.setattr(pl, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict({"camera_check": report} if k.get("check_cameras") else {},
                                                                   poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir))
    assert "check_cameras" not in calls[0] and not (out_dir / "camera_check.json").exists()
    pl.run_dataset(*args, out_dir=str(out_dir), check_cameras=dict(hypotheses=64))
    assert calls[1]["check_cameras"] == dict(hypotheses=64)
    assert json.load(open(out_dir / "camera_check.json")) == report
    pl.run_dataset(*args, check_cameras=True)
    assert calls[2]["check_cameras"] is True
