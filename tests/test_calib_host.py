"""CPU tests of the extrinsic refinement's rule and cases (include/lvba_hip.h "LiDAR-camera extrinsic refinement"):
csrc/calib_device.h on the host against the numpy oracle to the bit, the oracle's H and g against finite differences of its cost,
the held directions of the three trajectories, what the order of summation changes, and the default paths of run_full_pipeline and
run_dataset."""
import ctypes
import importlib
import sys

import numpy as np
import pytest

import calib_cases as cc
import calib_oracle as co
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/calib_device.h compiled for the host, without contraction (tests/calib_check.cpp)"""
    lib = ctypes.CDLL(build_check("calib_check", tmp_path_factory.mktemp("emul_calib")))
    P, I, L = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.emul_constants.argtypes = [P]
    lib.emul_constants.restype = None
    lib.emul_blocks.argtypes = [L]
    lib.emul_pairs.argtypes = [I, P, P, P, P]
    lib.emul_pairs.restype = None
    lib.emul_targets.argtypes = [L, P, P, P, P]
    lib.emul_targets.restype = None
    lib.emul_eval.argtypes = [L] + [P] * 12
    lib.emul_eval.restype = None
    lib.emul_sums.argtypes = [L] + [P] * 7 + [I, P]
    lib.emul_sums.restype = None
    lib.emul_step.argtypes = [P, P, I, P, P, P, P]
    lib.emul_jacobi.argtypes = [P, P, P]
    lib.emul_jacobi.restype = None
    lib.emul_solve.argtypes = [L, P, P, P, P, P, I, I, P, P, P, P, P]
    return lib


def ptr(a):
    return a.ctypes.data


def params(intr, o):
    return np.array([intr[0], intr[1], o["max_error_px"], o["loss_scale_px"], o["min_eig_ratio"], o["eps_rot"], o["eps_trans"],
                     o["min_records"], o["loss_kind"]], np.float64)


def prepared(emul, case):
    """(A, xy) of the host build, checked against the oracle's to the bit"""
    A = np.zeros((len(case["img_a"]), 12))
    emul.emul_pairs(len(A), ptr(case["poses"]), ptr(case["img_a"]), ptr(case["img_b"]), ptr(A))
    np.testing.assert_array_equal(A, co.pair_transforms(case["poses"], case["img_a"], case["img_b"]))
    xy = np.zeros((len(case["pair"]), 2))
    emul.emul_targets(len(xy), ptr(case["intr"]), ptr(case["uv"]), ptr(case["Xb"]), ptr(xy))
    np.testing.assert_array_equal(xy, co.targets(case["intr"], case["uv"], case["Xb"]))
    return A, xy


def host_solve(emul, case, reverse=False, **kw):
    o = co.options(**kw)
    A, xy = prepared(emul, case)
    R, t, s = case["R0"].copy(), case["t0"].copy(), np.zeros(co.NS)
    it, held = ctypes.c_int32(), ctypes.c_int32()
    st = emul.emul_solve(len(xy), ptr(A), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(params(case["intr"], o)), o["max_iterations"],
                         int(reverse), ptr(R), ptr(t), ptr(s), ctypes.addressof(it), ctypes.addressof(held))
    return dict(R=R, t=t, status=st, iterations=it.value, n_held=held.value, s=s)


def oracle_solve(case, **kw):
    return co.solve(case["poses"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"], case["R0"], case["t0"], **kw)


def test_partition_constants_are_the_ones_the_gpu_tests_read(emul):
    got = np.zeros(7, np.int64)
    emul.emul_constants(ptr(got))
    h = cc.header_constants()
    assert (h["CAL_NS"], h["CAL_BLOCK"], h["CAL_RUN"], h["CAL_MAX_BLOCKS"]) == tuple(got[:4]) and got[0] == co.NS
    per = h["CAL_BLOCK"] * h["CAL_RUN"]
    for n, want in ((0, 1), (1, 1), (per, 1), (per + 1, 2), (per * h["CAL_MAX_BLOCKS"], h["CAL_MAX_BLOCKS"]),
                    (per * h["CAL_MAX_BLOCKS"] + 1, h["CAL_MAX_BLOCKS"]), (10 ** 9, h["CAL_MAX_BLOCKS"])):
        assert emul.emul_blocks(n) == want


def test_device_header_on_the_host_equals_the_oracle(emul):
    """Record by record r, J and the weight, and the sums in both orders, bit for bit -- at the planted extrinsic, where residuals
    are tens of pixels and both branches of the Huber loss are taken, with unusable and behind-camera records among them, with
    and without the gate."""
    for case in (cc.general(), cc.noisy()):
        case = dict(case, uv=case["uv"].copy(), Xb=case["Xb"].copy())
        case["uv"][[3, 700]] = np.nan
        case["Xb"][[64, 5000]] = np.inf
        case["Xb"][[9, 1023]] *= -1.0                                             # behind both cameras
        A, xy = prepared(emul, case)
        assert np.isnan(xy[:, 0]).sum() == 4
        n = len(xy)
        for kw in (dict(), dict(max_error_px=4.0), dict(loss_kind=co.TRIVIAL)):
            o = co.options(**kw)
            e = co.evaluate(case["R0"], case["t0"], A, case["pair"], xy, case["Xb"], case["intr"], o)
            counted, r, J0, J1, rho = np.zeros(n, np.uint8), np.zeros((n, 2)), np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 3))
            p = params(case["intr"], o)
            emul.emul_eval(n, ptr(case["R0"]), ptr(case["t0"]), ptr(A), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p), ptr(counted),
                           ptr(r), ptr(J0), ptr(J1), ptr(rho))
            c = e["counted"]
            np.testing.assert_array_equal(counted.astype(bool), c)
            assert not c[[3, 700, 64, 5000, 9, 1023]].any() and c.sum() >= 0.3 * n
            if kw.get("max_error_px"):
                assert 0.05 * n < (~c).sum() < 0.95 * n                           # the gate cuts, and not everything
            if o["loss_kind"] == co.HUBER:
                assert 0.02 * n < (e["w"][c] < 1.0).sum() and (e["w"][c] == 1.0).sum() > (0 if case["name"] == "general" else 0.02 * n)
            np.testing.assert_array_equal(r[c], e["r"][c])
            np.testing.assert_array_equal(J0[c], e["J0"][c])
            np.testing.assert_array_equal(J1[c], e["J1"][c])
            np.testing.assert_array_equal(rho[c, 1], e["w"][c])
            np.testing.assert_array_equal(rho[c, 0], e["rho"][c])
            T = co.terms(e)
            for reverse in (0, 1):
                s = np.zeros(co.NS)
                emul.emul_sums(n, ptr(case["R0"]), ptr(case["t0"]), ptr(A), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p), reverse, ptr(s))
                np.testing.assert_array_equal(s, co.sums(T, bool(reverse)))
            np.testing.assert_array_equal(co.sums(T, prefixes=[0, 1, n])[[0, 2]], [np.zeros(co.NS), co.sums(T)])


def test_jacobi_with_vectors(emul):
    rng = np.random.default_rng(2)
    for k in range(20):
        B = rng.normal(size=(6, 6 if k % 2 else 4))
        H = B @ B.T                                                               # full rank, and rank 4
        lam, V = np.zeros(6), np.zeros((6, 6))
        emul.emul_jacobi(ptr(np.ascontiguousarray(H)), ptr(lam), ptr(V))
        lo, Vo = co.jacobi(H)
        np.testing.assert_array_equal(lam, lo)
        np.testing.assert_array_equal(V, Vo)
        scale = np.abs(H).max()
        assert np.abs(V @ V.T - np.eye(6)).max() < 1e-14
        assert np.abs(H @ V - V * lam).max() < 1e-13 * scale
        np.testing.assert_allclose(np.sort(lam), np.linalg.eigvalsh(H), atol=1e-13 * scale)


def test_gradient_and_hessian_against_finite_differences_of_the_cost():
    """g = sum rho' J^T r is the gradient of the cost at any extrinsic and under any loss -- checked at the planted one, where
    residuals are tens of pixels; H = sum rho' J^T J is its Hessian where the residuals vanish -- checked at the true extrinsic of
    the noise-free case.  Central differences along the exact perturbation Exp(om) R, Exp(om) t + up; steps 1e-5 (first) and 1e-3
    (second differences): truncation is O(step^2) relative, rounding 1e-16 cost / step^2 against |H| ~ 1e9."""
    case = cc.general()
    A = co.pair_transforms(case["poses"], case["img_a"], case["img_b"])
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    f = lambda R, t, o: co.cost(R, t, A, case["pair"], xy, case["Xb"], case["intr"], o)
    worst_g = 0.0
    for kw in (dict(loss_kind=co.TRIVIAL), dict(loss_scale_px=30.0)):
        o = co.options(**kw)
        s, _, _ = co.linearize(case["R0"], case["t0"], A, case["pair"], xy, case["Xb"], case["intr"], o)
        h = 1e-5
        fd = np.array([(f(*co.perturb(case["R0"], case["t0"], h * np.eye(6)[k]), o) - f(*co.perturb(case["R0"], case["t0"], -h * np.eye(6)[k]), o))
                       / (2 * h) for k in range(6)])
        worst_g = max(worst_g, np.abs(fd - s[co.G0:co.G0 + 6]).max() / np.abs(fd).max())
    o = co.options(loss_kind=co.TRIVIAL)
    R, t = case["R_true"], case["t_true"]
    s, _, _ = co.linearize(R, t, A, case["pair"], xy, case["Xb"], case["intr"], o)
    H = co.expand(s)
    h = 1e-3
    fd = np.zeros((6, 6))
    E = np.eye(6)
    for k in range(6):
        for l in range(k, 6):
            fd[k, l] = fd[l, k] = (f(*co.perturb(R, t, h * (E[k] + E[l])), o) - f(*co.perturb(R, t, h * (E[k] - E[l])), o)
                                   - f(*co.perturb(R, t, h * (E[l] - E[k])), o) + f(*co.perturb(R, t, -h * (E[k] + E[l])), o)) / (4 * h * h)
    worst_H = np.abs(fd - H).max() / np.abs(H).max()
    print("relative difference to central differences: g", worst_g, " H", worst_H)
    assert worst_g < 1e-6 and worst_H < 1e-4
    assert np.abs(s[co.G0:co.G0 + 6]).max() < 1e-6 * np.abs(H).max()              # and the true extrinsic is stationary


def test_held_directions_of_the_three_trajectories(emul):
    """General: none held, the planted 3 degrees / 10 cm recovered.  Screw: exactly the two the theory names.  Planar (a ground
    vehicle that moves across its axis): one.  The host build of the header and the oracle agree on every number."""
    for case, n_held in ((cc.general(), 0), (cc.screw(), 2), (cc.planar(), 1)):
        want, got = oracle_solve(case), host_solve(emul, case)
        assert got["status"] == want["status"] == co.CONVERGED and got["iterations"] == want["iterations"] <= 6
        np.testing.assert_array_equal(got["R"], want["R"])
        np.testing.assert_array_equal(got["t"], want["t"])
        assert got["n_held"] == want["n_held"] == n_held, case["name"]
        lam = want["eig"] / want["eig"].max()
        print(case["name"], "eigenvalues / largest:", lam)
        assert (lam[:n_held] < 1e-12).all() and (lam[n_held:] > 1e-4).all()      # the default ratio, 1e-6, lies well between
        U = cc.held_span(case["name"], want["R"], want["t"])
        if n_held:
            assert cc.principal_angles(U, want["vec"][want["held"]]).max() < 1e-6
        # the refined extrinsic is the true one up to a member Z of the unobservable family: X = X* Z
        Rt, tt = case["R_true"].reshape(3, 3), case["t_true"]
        Zr = co.left_difference(Rt.T @ want["R"].reshape(3, 3), np.zeros(3), np.eye(3), np.zeros(3))[:3]
        Zt = Rt.T @ (want["t"] - tt)
        free_rot = Zr if n_held < 2 else Zr[:2]                                   # screw: a turn about the body's z is free to stay
        free_trans = Zt if n_held == 0 else Zt[:2]
        assert np.linalg.norm(free_rot) < 1e-9 and np.linalg.norm(free_trans) < 1e-9, (case["name"], Zr, Zt)
        if n_held:
            # the held components do not move: second order in the distance moved at most (the held span turns with the extrinsic)
            d0 = co.left_difference(want["R"], want["t"], case["R0"], case["t0"])
            assert np.abs(want["vec"][want["held"]] @ d0).max() <= d0 @ d0


def test_order_of_summation_on_the_noisy_case(emul):
    """0.5 px of noise and 20 % gross outliers under the default Huber loss: what the order of summation alone changes in the
    refined extrinsic (calib_cases.NOISY_ORDER_D), and how near the planted extrinsic the rule comes."""
    case = cc.noisy()
    a, b = oracle_solve(case), oracle_solve(case, reverse=True)
    ha, hb = host_solve(emul, case), host_solve(emul, case, reverse=True)
    for o, h in ((a, ha), (b, hb)):
        np.testing.assert_array_equal(h["R"], o["R"])
        np.testing.assert_array_equal(h["t"], o["t"])
    assert a["status"] == b["status"] == co.CONVERGED and a["iterations"] == b["iterations"]
    d = max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max())
    err = co.left_difference(a["R"], a["t"], case["R_true"], case["t_true"])
    print("index order against reversed order:", d, "; error against the planted extrinsic: %.4f deg, %.2f mm; rmse %.2f px"
          % (np.degrees(np.linalg.norm(err[:3])), 1e3 * np.linalg.norm(err[3:]), a["rmse_px"]))
    assert d <= cc.NOISY_ORDER_D
    assert np.degrees(np.linalg.norm(err[:3])) < 0.05 and np.linalg.norm(err[3:]) < 0.005
    assert 0.15 < case["outlier"].mean() < 0.25


def test_status_rules(emul):
    o = co.options()
    s = np.zeros(co.NS)
    res, cnt = np.zeros(45), np.zeros(2, np.int32)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    s[co.CNT] = 99
    assert emul.emul_step(ptr(s), ptr(params(cc.INTR, o)), 1, ptr(R), ptr(t), ptr(res), ptr(cnt)) == co.TOO_FEW_RECORDS
    s[co.CNT] = 100                                                                # H = 0: no direction is observable
    assert emul.emul_step(ptr(s), ptr(params(cc.INTR, o)), 1, ptr(R), ptr(t), ptr(res), ptr(cnt)) == co.DEGENERATE and cnt[0] == 6
    assert co.step(s, o, True, R, t)[0] == co.DEGENERATE
    k = 0
    for a in range(6):
        for b in range(a, 6):
            s[k] = 4.0 if a == b else 0.0
            k += 1
    s[co.G0] = 1.0
    assert emul.emul_step(ptr(s), ptr(params(cc.INTR, o)), 0, ptr(R), ptr(t), ptr(res), ptr(cnt)) == co.MAX_ITERATIONS
    np.testing.assert_array_equal(R, np.eye(3).reshape(9))
    assert emul.emul_step(ptr(s), ptr(params(cc.INTR, o)), 1, ptr(R), ptr(t), ptr(res), ptr(cnt)) == co.RUNNING and cnt[0] == 0
    np.testing.assert_array_equal(R, co.retract(np.eye(3).reshape(9), np.zeros(3), np.r_[-0.25, 0, 0, 0, 0, 0])[0])
    s[co.G0] = 1e-12
    assert emul.emul_step(ptr(s), ptr(params(cc.INTR, o)), 1, ptr(R), ptr(t), ptr(res), ptr(cnt)) == co.CONVERGED


class _FakeScans:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


def test_run_full_pipeline_without_the_keyword_is_the_untouched_path(monkeypatch):
    """calibrate_extrinsic=False (the default) hands the visual stage exactly what the call without the keyword hands it, and
    neither imports the calib module nor looks a new entry point up."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")

    class NoCalibLib:
        def __getattr__(self, name):
            if name.startswith("lvba_calib"):
                pytest.fail(f"{name} looked up on the default path")
            raise AttributeError(name)

    calls = []
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(pl, "_calibrate_extrinsic", lambda *a, **k: pytest.fail("the calibration ran on the default path"))
    monkeypatch.setattr(L, "load", lambda: NoCalibLib())
    sys.modules.pop("global-lvba_amd.calib", None)
    kps = [np.zeros((5, 2), np.float32)] * 2
    args = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
            np.ones(8), 640, 512, kps, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])
    out0 = pl.run_full_pipeline(*args, enable_lidar_ba=False)
    out1 = pl.run_full_pipeline(*args, enable_lidar_ba=False, calibrate_extrinsic=False)
    assert "global-lvba_amd.calib" not in sys.modules
    (a0, k0), (a1, k1) = calls
    assert k0.keys() == k1.keys() and len(a0) == len(a1)
    for x, y in zip(a0[1:], a1[1:]):
        assert repr(x) == repr(y)
    assert "extrinsic" not in out0 and "extrinsic" not in out1
    with pytest.raises(ValueError, match="apply"):
        pl.run_full_pipeline(*args, enable_lidar_ba=False, calibrate_extrinsic="apply")   # no depth images from the matching stage


def test_run_full_pipeline_reports_or_applies(monkeypatch):
    """True reports and hands the visual stage the configured extrinsic; "apply" hands it the refined one and closes the matching
    stage's depth images first."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    closed = []

    class Depth:
        def close(self):
            closed.append(self)

    Rn, tn = co.rodrigues([0.0, 0.0, 0.1]), np.array([0.1, 0.2, 0.3])
    calls = []
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl.V.DepthImages, "render", staticmethod(lambda *a, **k: Depth()))
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(pl, "_calibrate_extrinsic", lambda *a, **k: dict(status="converged", Rci=Rn.tolist(), tci=tn.tolist(), kw=sorted(k)))
    kps = [np.zeros((5, 2), np.float32)] * 2
    args = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
            np.ones(8), 640, 512, kps, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])
    fn = lambda cams, depth=None: ([(0, 1)], [np.array([[0, 1]], np.int32)])
    out = pl.run_full_pipeline(*args, enable_lidar_ba=False, match_fn=fn, match_depth=True, calibrate_extrinsic=dict(rounds=2))
    assert out["extrinsic"]["applied"] is False and "rounds" in out["extrinsic"]["kw"]
    np.testing.assert_array_equal(calls[0][0][6], np.eye(3))
    assert calls[0][1]["depth"] is not None and len(closed) == 1
    out = pl.run_full_pipeline(*args, enable_lidar_ba=False, match_fn=fn, match_depth=True, calibrate_extrinsic="apply")
    assert out["extrinsic"]["applied"] is True
    np.testing.assert_array_equal(calls[1][0][6], Rn)
    np.testing.assert_array_equal(calls[1][0][7], tn)
    assert "depth" not in calls[1][1] and len(closed) == 2


def test_calibration_records_use_both_directions_in_order(monkeypatch):
    pl = importlib.import_module("global-lvba_amd.pipeline")
    RS = importlib.import_module("global-lvba_amd.resect")
    nan = np.nan
    points = [np.array([[1., 0, 0], [nan, nan, nan], [3, 0, 0]]), np.array([[10., 0, 0], [11, 0, 0]]), np.array([[nan, nan, nan]])]
    kps = [np.array([[0., 0], [1, 1], [2, 2]]), np.array([[10., 10], [11, 11]]), np.array([[20., 20]])]
    pairs = [(1, 0), (0, 2)]
    matches = [np.array([[0, 2], [1, 1], [1, 0]]), np.array([[2, 0]])]
    Rcw = np.stack([co.rodrigues([0, 0, 0.1 * k]) for k in range(3)])
    tcw = np.array([[0., 0, 1], [0, 2, 0], [3, 0, 0]])
    monkeypatch.setattr(RS, "lift_keypoints", lambda depth, uv, intr, R, t: points)
    rec, (ia, ib) = pl.calibration_records(kps, pairs, matches, object(), Rcw, tcw, np.ones(8))
    # the order of correspondences_from_matches: pair (1, 0) image 1's side, then image 0's; pair (0, 2) image 0's side, then image 2's
    np.testing.assert_array_equal(ia, [1, 0, 0, 2])
    np.testing.assert_array_equal(ib, [0, 1, 2, 0])
    np.testing.assert_array_equal(rec["pair"], [0, 0, 1, 1, 1, 3])
    np.testing.assert_array_equal(rec["uv"], [[10, 10], [11, 11], [2, 2], [1, 1], [0, 0], [20, 20]])
    world = np.array([[3., 0, 0], [1, 0, 0], [10, 0, 0], [11, 0, 0], [11, 0, 0], [3, 0, 0]])
    src = [0, 0, 1, 1, 1, 0]
    np.testing.assert_array_equal(rec["Xb"], np.stack([Rcw[s] @ w + tcw[s] for s, w in zip(src, world)]))
    assert rec["pair"].dtype == np.int32 and rec["uv"].dtype == np.float32 and rec["Xb"].dtype == np.float64
    kp, X = pl.correspondences_from_matches(pairs, matches, points)               # the same matches, image by image
    assert sum(len(k) for k in kp) == len(rec["pair"])
    rec, (ia, ib) = pl.calibration_records(kps, [], [], object(), Rcw, tcw, np.ones(8))
    assert rec["pair"].shape == (0,) and rec["uv"].shape == (0, 2) and rec["Xb"].shape == (0, 3) and len(ia) == 0


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
    calls = []
    report = dict(status="too_few_records", n_used=2, n_held=0, Rci=np.eye(3).tolist(), tci=[0.0, 0.0, 0.0], applied=False, rounds=[])
    monkeypatch.setattr(pl, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict({"extrinsic": report} if k.get("calibrate_extrinsic") else {},
                                                                   poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir))
    assert "calibrate_extrinsic" not in calls[0] and not (out_dir / "extrinsic.json").exists()
    pl.run_dataset(*args, out_dir=str(out_dir), calibrate_extrinsic=dict(rounds=2))
    assert calls[1]["calibrate_extrinsic"] == dict(rounds=2)
    assert json.load(open(out_dir / "extrinsic.json")) == report
    pl.run_dataset(*args, calibrate_extrinsic="apply")
    assert calls[2]["calibrate_extrinsic"] == "apply"


def test_summary_is_plain_python_and_names_the_held_directions():
    CB = importlib.import_module("global-lvba_amd.calib")
    case = cc.screw()
    r = oracle_solve(case)
    rep = dict(Rci=r["R"].reshape(3, 3), tci=r["t"], status=r["status"], iterations=r["iterations"], n_used=r["n_used"], rmse_px=0.5,
               cost=r["cost"], n_held=r["n_held"], eigenvalues=r["eig"], eigenvectors=r["vec"], information=r["information"])
    s = CB.summary(rep, case["R0"], case["t0"])
    import json
    json.dumps(s)
    assert s["status"] == "converged" and s["n_held"] == 2 and len(s["held"]) == 2
    moved = co.left_difference(r["R"], r["t"], case["R0"], case["t0"])
    assert s["rotation_deg"] == pytest.approx(np.degrees(np.linalg.norm(moved[:3])), rel=1e-9)
    assert s["translation_m"] == pytest.approx(np.linalg.norm(r["t"] - case["t0"]), rel=1e-12)
    assert 0.5 < s["rotation_deg"] <= cc.PLANT_ROT_DEG * 1.01                   # a part of the planted turn is about the held axis
    free = r["vec"][2:]
    cov = 0.25 * (free.T / r["eig"][2:]) @ free
    assert s["std_rot_deg"] == pytest.approx(np.degrees(np.sqrt(np.trace(cov[:3, :3])))) and s["std_trans_m"] == pytest.approx(np.sqrt(np.trace(cov[3:, 3:])))
    assert CB.best_job(dict(status=np.array([1, 0, 0, 3]), cost=np.array([0.1, 2.0, 2.0, 0.0]))) == 1
    assert CB.best_job(dict(status=np.array([2]), cost=np.array([0.0]))) is None
