"""CPU tests of the time offset's rule and cases (include/lvba_hip.h "the camera-LiDAR time offset", DESIGN.md §10o "time offset"):
csrc/calib_td_device.h on the host against the numpy oracle to the bit, the seventh column against central differences of the
oracle's residual, the held sets of the trajectories, zero twists against the 6-parameter rule's bits, the status rules, what the
order of summation changes, pipeline.body_twists, calib.shift_poses and the pipeline's default path."""
import ctypes
import importlib
import sys

import numpy as np
import pytest

import calib_cases as cc
import calib_oracle as co
import calib_td_cases as tc
import calib_td_oracle as cto
from host_build import build_check

P, I, L64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
TDS = (0.0, 0.013, -0.05)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/calib_td_device.h compiled for the host, without contraction (tests/calib_td_check.cpp)"""
    lib = ctypes.CDLL(build_check("calib_td_check", tmp_path_factory.mktemp("emul_calib_td")))
    lib.emul_td_constants.argtypes = [P]
    lib.emul_td_constants.restype = None
    lib.emul_td_shift.argtypes = [I, P, P, D, P]
    lib.emul_td_shift.restype = None
    lib.emul_td_pairs.argtypes = [I, P, P, P, P, D, P]
    lib.emul_td_pairs.restype = None
    lib.emul_td_eval.argtypes = [L64] + [P] * 12
    lib.emul_td_eval.restype = None
    lib.emul_td_sums.argtypes = [L64] + [P] * 6 + [I, P]
    lib.emul_td_sums.restype = None
    lib.emul_td_step.argtypes = [P, P, I, P, P, P]
    lib.emul_td_solve.argtypes = [I, P, P, P, P, L64, P, P, P, P, I, I, P, P, P, P, P]
    return lib


@pytest.fixture(scope="module")
def emul6(tmp_path_factory):
    """the 6-parameter header on the host (tests/calib_check.cpp), for the zero-twist comparison"""
    lib = ctypes.CDLL(build_check("calib_check", tmp_path_factory.mktemp("emul_calib6")))
    lib.emul_pairs.argtypes = [I, P, P, P, P]
    lib.emul_pairs.restype = None
    lib.emul_sums.argtypes = [L64] + [P] * 7 + [I, P]
    lib.emul_sums.restype = None
    lib.emul_solve.argtypes = [L64, P, P, P, P, P, I, I, P, P, P, P, P]
    return lib


def ptr(a):
    return a.ctypes.data


def params(intr, o):
    return np.array([intr[0], intr[1], o["max_error_px"], o["loss_scale_px"], o["min_eig_ratio"], o["eps_rot"], o["eps_trans"],
                     o["min_records"], o["loss_kind"], o["eps_td_s"], o["max_abs_td_s"]], np.float64)


def host_table(emul, case, td):
    E = np.zeros((len(case["img_a"]), cto.ROW))
    emul.emul_td_pairs(len(E), ptr(case["poses"]), ptr(case["twists"]), ptr(case["img_a"]), ptr(case["img_b"]), td, ptr(E))
    return E


def host_solve(emul, case, td0=0.0, reverse=False, R0=None, t0=None, **kw):
    o = cto.options(**kw)
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    x = np.r_[case["R0"] if R0 is None else R0, case["t0"] if t0 is None else t0, td0].astype(np.float64)
    s, ev = np.zeros(cto.NS), np.zeros(56)
    it, held = ctypes.c_int32(), ctypes.c_int32()
    st = emul.emul_td_solve(len(case["img_a"]), ptr(case["poses"]), ptr(case["twists"]), ptr(case["img_a"]), ptr(case["img_b"]), len(xy),
                            ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(params(case["intr"], o)), o["max_iterations"], int(reverse),
                            ptr(x), ptr(s), ctypes.addressof(it), ctypes.addressof(held), ptr(ev))
    return dict(R=x[:9].copy(), t=x[9:12].copy(), td=float(x[12]), status=st, iterations=it.value, n_held=held.value, s=s, eig=ev[:7].copy(),
                vec=ev[7:].reshape(7, 7).copy())


def oracle_solve(case, td0=0.0, **kw):
    return cto.solve(case["poses"], case["twists"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"],
                     case["R0"], case["t0"], td0, **kw)


def same_run(got, want):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] and got["n_held"] == want["n_held"]
    np.testing.assert_array_equal(got["R"], want["R"])
    np.testing.assert_array_equal(got["t"], want["t"])
    assert got["td"] == want["td"]
    np.testing.assert_array_equal(got["s"], want["s"])
    np.testing.assert_array_equal(got["eig"], want["eig"])
    np.testing.assert_array_equal(got["vec"], want["vec"])


def test_constants_are_the_ones_the_tests_read(emul):
    got = np.zeros(8, np.int64)
    emul.emul_td_constants(ptr(got))
    h = tc.header_constants()
    assert (h["CAL_TD_N"], h["CAL_TD_NS"], h["CAL_TD_ROW"], h["CAL_TD_EXT"]) == tuple(got[[0, 1, 2, 4]]) and got[3] == 2 * 49 + 2 * 7
    assert (got[0], got[1], got[2], got[7]) == (cto.N, cto.NS, cto.ROW, cto.OUT_OF_RANGE) and h["CAL_BLOCK"] == 256
    hdr = open(__file__.replace("tests/test_calib_td_host.py", "include/lvba_hip.h")).read()
    assert "#define LVBA_CALIB_TD_SUMS 39" in hdr and "#define LVBA_CALIB_TD_OUT_OF_RANGE 4" in hdr


def test_pair_table_and_shifted_poses_equal_the_oracle(emul):
    """A, om' and dv at td = 0, 0.013 and -0.05, and the shifted poses themselves, bit for bit; the shifted rotation is a rotation
    about om by 2 atan(td |om| / 2); calib.shift_poses states the same motion."""
    CB = importlib.import_module("global-lvba_amd.calib")
    for case in (tc.general(), tc.planar(), tc.screw()):
        for td in TDS:
            S = np.zeros_like(case["poses"])
            emul.emul_td_shift(len(S), ptr(case["poses"]), ptr(case["twists"]), td, ptr(S))
            want = cto.shift_poses(case["poses"], case["twists"], td)
            np.testing.assert_array_equal(S, want)
            np.testing.assert_array_equal(host_table(emul, case, td), cto.pair_table(case["poses"], case["twists"], case["img_a"], case["img_b"], td))
            np.testing.assert_allclose(CB.shift_poses(case["poses"], case["twists"], td), want, rtol=0, atol=1e-15)
            for k in range(len(S)):
                om = case["twists"][k, :3]
                n = np.linalg.norm(om)
                exact = case["poses"][k, :9].reshape(3, 3) @ co.rodrigues(om / n * 2.0 * np.arctan(0.5 * td * n))
                assert np.abs(S[k, :9].reshape(3, 3) - exact).max() < 1e-15
        np.testing.assert_array_equal(cto.shift_poses(case["poses"], case["twists"], 0.0), case["poses"])
    with pytest.raises(ValueError):
        CB.shift_poses(np.zeros((3, 12)), np.zeros((2, 6)), 0.1)


def test_device_header_on_the_host_equals_the_oracle(emul):
    """Record by record r, both 7-entry rows and the loss, and the sums in both orders, bit for bit -- at the planted extrinsic and
    td = 0.013, with unusable and behind-camera records among them, with and without the gate."""
    for case in (tc.general(), tc.noisy()):
        case = dict(case, uv=case["uv"].copy(), Xb=case["Xb"].copy())
        case["uv"][[3, 700]] = np.nan
        case["Xb"][[64, 5000]] = np.inf
        case["Xb"][[9, 1023]] *= -1.0                                             # behind both cameras
        xy = co.targets(case["intr"], case["uv"], case["Xb"])
        n = len(xy)
        td = 0.013
        E = host_table(emul, case, td)
        x = np.r_[case["R0"], case["t0"], td]
        for kw in (dict(), dict(max_error_px=4.0), dict(loss_kind=co.TRIVIAL)):
            o = cto.options(**kw)
            e = cto.evaluate(case["R0"], case["t0"], E, case["pair"], xy, case["Xb"], case["intr"], o)
            counted, r, J0, J1, rho = np.zeros(n, np.uint8), np.zeros((n, 2)), np.zeros((n, 7)), np.zeros((n, 7)), np.zeros((n, 3))
            p = params(case["intr"], o)
            emul.emul_td_eval(n, ptr(case["R0"]), ptr(case["t0"]), ptr(E), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p), ptr(counted),
                              ptr(r), ptr(J0), ptr(J1), ptr(rho))
            c = e["counted"]
            np.testing.assert_array_equal(counted.astype(bool), c)
            assert not c[[3, 700, 64, 5000, 9, 1023]].any() and c.sum() >= 0.3 * n
            np.testing.assert_array_equal(r[c], e["r"][c])
            np.testing.assert_array_equal(J0[c], e["J0"][c])
            np.testing.assert_array_equal(J1[c], e["J1"][c])
            np.testing.assert_array_equal(rho[c, 1], e["w"][c])
            np.testing.assert_array_equal(rho[c, 0], e["rho"][c])
            assert np.abs(J0[c, 6]).max() > 1.0                                   # the new column is there
            T = cto.terms(e)
            for reverse in (0, 1):
                s = np.zeros(cto.NS)
                emul.emul_td_sums(n, ptr(x), ptr(E), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p), reverse, ptr(s))
                np.testing.assert_array_equal(s, cto.sums(T, bool(reverse)))


def test_seventh_column_against_central_differences():
    """J[6] against central differences of the oracle's residual along td, h = 1e-6, at td = 0.013, on two trajectories: within 1e-8
    of the largest entry (the prototype measured at most 2.7e-10; the margin covers the quotient's own rounding, eps |r| / h).
    Measured here: 2.8e-10 (general) and 1.8e-10 (planar)."""
    h, td = 1e-6, 0.013
    for case in (tc.general(), tc.planar()):
        xy = co.targets(case["intr"], case["uv"], case["Xb"])
        o = cto.options()
        ev = lambda x: cto.evaluate(case["R0"], case["t0"], cto.pair_table(case["poses"], case["twists"], case["img_a"], case["img_b"], x),
                                    case["pair"], xy, case["Xb"], case["intr"], o)
        e, ep, em = ev(td), ev(td + h), ev(td - h)
        c = e["counted"] & ep["counted"] & em["counted"]
        assert c.mean() > 0.9
        fd = (ep["r"][c] - em["r"][c]) / (2 * h)
        J6 = np.stack([e["J0"][c, 6], e["J1"][c, 6]], 1)
        rel = np.abs(fd - J6).max() / np.abs(J6).max()
        print(case["name"], "J[6] against central differences, relative to the largest entry:", rel, "; largest entry", np.abs(J6).max())
        assert rel < 1e-8


def test_held_sets_and_recovery(emul):
    """General: none held, 3 degrees / 10 cm / 0 s off recovered with td.  Planar with varying twists: only the translation along
    the axis is held, td is recovered.  One constant body-frame twist: the screw's two directions and the td axis.  The host build
    and the oracle agree on every number."""
    for case, n_held in ((tc.general(), 0), (tc.general(-0.05), 0), (tc.planar(), 1), (tc.screw(), 3)):
        want, got = oracle_solve(case), host_solve(emul, case)
        same_run(got, want)
        lam = want["eig"] / want["eig"].max()
        print(case["name"], case["td_true"], "iterations", want["iterations"], "rmse", want["rmse_px"], "td", want["td"], "eigenvalues / largest:", lam)
        assert want["status"] == co.CONVERGED and want["n_held"] == n_held and want["iterations"] <= 8
        assert (lam[:n_held] < 1e-12).all() and (lam[n_held:] > 1e-5).all()      # the default ratio, 1e-6, lies between
        Rt, tt = case["R_true"].reshape(3, 3), case["t_true"]
        Zr = co.left_difference(Rt.T @ want["R"].reshape(3, 3), np.zeros(3), np.eye(3), np.zeros(3))[:3]
        Zt = Rt.T @ (want["t"] - tt)
        if case["name"] == "general":
            print("  error", np.linalg.norm(Zr), "rad", np.linalg.norm(Zt), "m", abs(want["td"] - case["td_true"]), "s")
            assert np.linalg.norm(Zr) <= 1e-9 and np.linalg.norm(Zt) <= 1e-9 and abs(want["td"] - case["td_true"]) <= 1e-9
        elif case["name"] == "planar":
            held = want["vec"][0]
            assert cc.principal_angles(np.r_[cc.held_span("planar", want["R"], want["t"])[0], 0.0][None], held[None]).max() < 1e-6
            print("  free error", np.linalg.norm(Zr), np.linalg.norm(Zt[:2]), abs(want["td"] - case["td_true"]), "held part", Zt[2])
            assert np.linalg.norm(Zr) <= 1e-9 and np.linalg.norm(Zt[:2]) <= 1e-9 and abs(want["td"] - case["td_true"]) <= 1e-9
        else:
            U = tc.screw_held_span(case, want["R"], want["t"])
            assert cc.principal_angles(U, want["vec"][:3]).max() < 1e-6
            assert cc.principal_angles(want["vec"][:3], np.eye(7)[6:]).max() < 1e-6   # the td axis lies in the held span
            assert abs(want["td"]) <= 1e-12


def test_constant_twist_leaves_the_pair_table_independent_of_td(emul):
    """poses exp(k dt xi) with that twist at every image: A(td) is A(0) up to rounding and J[6] vanishes (the prototype measured
    max |J[6]| = 3.4e-13; measured here 1.8e-13 against entries of 2e2 in the other columns)"""
    case = tc.screw()
    E0, E1 = host_table(emul, case, 0.0), host_table(emul, case, 0.05)
    assert np.abs(E1[:, :12] - E0[:, :12]).max() < 1e-15
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    e = cto.evaluate(case["R0"], case["t0"], E1, case["pair"], xy, case["Xb"], case["intr"], cto.options())
    c = e["counted"]
    worst = max(np.abs(e["J0"][c, 6]).max(), np.abs(e["J1"][c, 6]).max())
    print("constant twist: max |J[6]|", worst, "against", np.abs(e["J0"][c, :6]).max())
    assert worst < 1e-11 and np.abs(e["J0"][c, :6]).max() > 100.0
    got = host_solve(emul, case, td0=0.01)
    assert got["status"] == co.CONVERGED and got["n_held"] == 3 and abs(got["td"] - 0.01) <= 1e-12


def test_zero_twists_are_the_six_parameter_rule(emul, emul6):
    """J[6] is exactly 0 and cal_jacobi skips zero pivots: the 6 x 6 block of every sum, the extrinsic, the status and the iteration
    count equal the 6-parameter host build's bits; td comes back as it went in; one more direction is held."""
    case = tc.zero()
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    A = np.zeros((len(case["img_a"]), 12))
    emul6.emul_pairs(len(A), ptr(case["poses"]), ptr(case["img_a"]), ptr(case["img_b"]), ptr(A))
    o = cto.options()
    p = params(case["intr"], o)
    i6 = [k for k, (a, b) in enumerate((a, b) for a in range(7) for b in range(a, 7)) if b < 6]
    assert len(i6) == 21
    for td0 in (0.0, 0.04):
        E = host_table(emul, case, td0)
        np.testing.assert_array_equal(E[:, :12], A)
        assert not E[:, 12:].any()
        s7, s6 = np.zeros(cto.NS), np.zeros(co.NS)
        x = np.r_[case["R0"], case["t0"], td0]
        emul.emul_td_sums(len(xy), ptr(x), ptr(E), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p), 0, ptr(s7))
        emul6.emul_sums(len(xy), ptr(case["R0"]), ptr(case["t0"]), ptr(A), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p[:9].copy()), 0, ptr(s6))
        np.testing.assert_array_equal(s7[i6], s6[:21])
        np.testing.assert_array_equal(s7[cto.G0:cto.G0 + 6], s6[co.G0:co.G0 + 6])
        np.testing.assert_array_equal(s7[cto.COST:], s6[co.COST:])
        assert not s7[[6, 12, 17, 21, 24, 26, 27, cto.G0 + 6]].any()
        got = host_solve(emul, case, td0=td0)
        R, t, s = case["R0"].copy(), case["t0"].copy(), np.zeros(co.NS)
        it, held = ctypes.c_int32(), ctypes.c_int32()
        st = emul6.emul_solve(len(xy), ptr(A), ptr(case["pair"]), ptr(xy), ptr(case["Xb"]), ptr(p[:9].copy()), o["max_iterations"], 0, ptr(R),
                              ptr(t), ptr(s), ctypes.addressof(it), ctypes.addressof(held))
        assert (got["status"], got["iterations"], got["n_held"]) == (st, it.value, held.value + 1) and st == co.CONVERGED
        np.testing.assert_array_equal(got["R"], R)
        np.testing.assert_array_equal(got["t"], t)
        assert got["td"] == td0
        same_run(got, oracle_solve(case, td0))


def test_order_of_summation_on_the_noisy_case(emul):
    """0.5 px of noise and 20 % gross outliers under the default Huber loss: what the order of summation alone changes in the
    refined (R, t, td) (calib_td_cases.NOISY_ORDER_D), and how near the truth the rule comes."""
    case = tc.noisy()
    a, b = oracle_solve(case), oracle_solve(case, reverse=True)
    ha, hb = host_solve(emul, case), host_solve(emul, case, reverse=True)
    same_run(ha, a)
    same_run(hb, b)
    assert a["status"] == b["status"] == co.CONVERGED and a["iterations"] == b["iterations"] and a["n_held"] == 0
    d = max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["td"] - b["td"]))
    err = co.left_difference(a["R"], a["t"], case["R_true"], case["t_true"])
    print("index order against reversed order:", d, "; error against the truth: %.4f deg, %.2f mm, %.3f ms; rmse %.2f px"
          % (np.degrees(np.linalg.norm(err[:3])), 1e3 * np.linalg.norm(err[3:]), 1e3 * abs(a["td"] - case["td_true"]), a["rmse_px"]))
    assert d <= tc.NOISY_ORDER_D
    assert np.degrees(np.linalg.norm(err[:3])) < 0.05 and np.linalg.norm(err[3:]) < 0.005 and abs(a["td"] - case["td_true"]) < 0.002


def test_the_six_parameter_rule_absorbs_an_offset_the_seventh_gives_back():
    """started at the true extrinsic with 20 ms planted, the 6-parameter rule walks away from it; with td it stays"""
    case = tc.general()
    six = co.solve(case["poses"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"], case["R_true"], case["t_true"])
    e6 = co.left_difference(six["R"], six["t"], case["R_true"], case["t_true"])
    seven = cto.solve(case["poses"], case["twists"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"],
                      case["R_true"], case["t_true"], 0.0)
    e7 = co.left_difference(seven["R"], seven["t"], case["R_true"], case["t_true"])
    print("6 parameters: %.3f deg %.3f m rmse %.2f px; 7: %.2e rad %.2e m rmse %.2e px" % (
        np.degrees(np.linalg.norm(e6[:3])), np.linalg.norm(e6[3:]), six["rmse_px"], np.linalg.norm(e7[:3]), np.linalg.norm(e7[3:]), seven["rmse_px"]))
    assert np.degrees(np.linalg.norm(e6[:3])) > 0.1 and six["rmse_px"] > 1.0
    assert np.linalg.norm(e7) < 1e-9 and seven["rmse_px"] < 1e-6 and abs(seven["td"] - 0.02) < 1e-9


def test_status_rules(emul):
    o = cto.options()
    p = params(cc.INTR, o)
    s = np.zeros(cto.NS)
    res, cnt = np.zeros(59), np.zeros(1, np.int32)
    x0 = np.r_[np.eye(3).reshape(9), np.zeros(3), 0.01]
    x = x0.copy()
    s[cto.CNT] = 99
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == co.TOO_FEW_RECORDS
    s[cto.CNT] = 100                                                               # H = 0: no direction is observable
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == co.DEGENERATE and cnt[0] == 7
    assert cto.step(s, o, True, x[:9], x[9:12], x[12])[0] == co.DEGENERATE
    k = 0
    for a in range(7):
        for b in range(a, 7):
            s[k] = 4.0 if a == b else 0.0
            k += 1
    s[cto.G0 + 6] = 0.1                                                            # d[6] = -0.025
    assert emul.emul_td_step(ptr(s), ptr(p), 0, ptr(x), ptr(res), ptr(cnt)) == co.MAX_ITERATIONS
    np.testing.assert_array_equal(x, x0)
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == co.RUNNING and cnt[0] == 0
    assert x[12] == 0.01 + -0.025 and cto.step(s, o, True, x0[:9], x0[9:12], x0[12])[3] == x[12]
    s[cto.G0 + 6] = 1e-9                                                           # the rotation and the translation stand, td still moves
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == co.RUNNING
    s[cto.G0 + 6] = 1e-12
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == co.CONVERGED
    s[cto.G0 + 6] = -1.0                                                           # d[6] = 0.25: past max_abs_td_s
    before = x.copy()
    assert emul.emul_td_step(ptr(s), ptr(p), 1, ptr(x), ptr(res), ptr(cnt)) == cto.OUT_OF_RANGE
    np.testing.assert_array_equal(x, before)
    assert cto.step(s, o, True, x[:9], x[9:12], x[12])[0] == cto.OUT_OF_RANGE


def test_an_offset_past_the_bound_returns_the_start_values(emul):
    """td_true = 0.3 under the default bound of 0.2 s: OUT_OF_RANGE, and (R, t, td) come back bit for bit"""
    case = tc.general(0.3)
    want, got = oracle_solve(case), host_solve(emul, case)
    same_run(got, want)
    assert got["status"] == cto.OUT_OF_RANGE and got["td"] == 0.0
    np.testing.assert_array_equal(got["R"], case["R0"])
    np.testing.assert_array_equal(got["t"], case["t0"])
    wide = host_solve(emul, case, max_abs_td_s=0.5)
    assert wide["status"] == co.CONVERGED and abs(wide["td"] - 0.3) < 1e-9


def test_body_twists_on_an_analytic_trajectory():
    """scans on a constant screw: every image gets that twist (om in the body frame, v in the world frame of its segment); images
    outside the scans take the end segments"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    om, u = np.array([0.1, -0.2, 0.3]), np.array([0.5, 0.2, -0.1])
    ts = 10.0 + 0.1 * np.arange(6)
    poses = np.zeros((6, 12))
    for k, t in enumerate(ts):
        poses[k, :9], poses[k, 9:] = co.rodrigues((t - 10.0) * om).reshape(9), (t - 10.0) * u
    img_t = np.array([9.9, 10.0, 10.05, 10.27, 10.5, 10.8])
    tw = pl.body_twists(poses, ts, img_t)
    assert tw.shape == (6, 6)
    np.testing.assert_allclose(tw[:, :3], np.tile(om, (6, 1)), atol=1e-12)
    np.testing.assert_allclose(tw[:, 3:], np.tile(u, (6, 1)), atol=1e-12)
    # two segments of different motion: an image takes its own segment's
    poses[2, 9:] = poses[1, 9:] + 0.1 * np.array([0.0, 1.0, 0.0])
    tw = pl.body_twists(poses[:3], ts[:3], np.array([10.05, 10.15]))
    np.testing.assert_allclose(tw[0, 3:], u, atol=1e-12)
    np.testing.assert_allclose(tw[1, 3:], [0.0, 1.0, 0.0], atol=1e-12)
    with pytest.raises(ValueError):
        pl.body_twists(poses[:1], ts[:1], img_t)


def test_summary_reports_the_offset_and_its_deviation():
    CB = importlib.import_module("global-lvba_amd.calib")
    case = tc.general()
    r = oracle_solve(case)
    rep = dict(Rci=r["R"].reshape(3, 3), tci=r["t"], td=r["td"], status=r["status"], iterations=r["iterations"], n_used=r["n_used"], rmse_px=0.5,
               cost=r["cost"], n_held=r["n_held"], eigenvalues=r["eig"], eigenvectors=r["vec"], information=r["information"])
    s = CB.summary(rep, case["R0"], case["t0"])
    import json
    json.dumps(s)
    cov = 0.25 * np.linalg.inv(r["information"])
    assert s["time_offset_s"] == r["td"] and s["std_td_s"] == pytest.approx(np.sqrt(cov[6, 6]), rel=1e-6)
    assert s["std_trans_m"] == pytest.approx(np.sqrt(np.trace(cov[3:6, 3:6])), rel=1e-6) and s["held"] == []
    six = dict(rep, eigenvalues=r["eig"][1:], eigenvectors=np.eye(6), information=np.eye(6))
    six.pop("td")
    s6 = CB.summary(six, case["R0"], case["t0"])
    assert s6["time_offset_s"] is None and s6["std_td_s"] is None
    assert "td_out_of_range" == CB.STATUS_NAMES[CB.TD_OUT_OF_RANGE]


class _FakeScans:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


def test_the_default_path_looks_no_td_symbol_up(monkeypatch):
    """calibrate_extrinsic without time_offset calls calib.refine_extrinsic with the arguments it always had and never touches a
    _td entry point; with time_offset it shifts the poses the records are lifted at, hands the solver the ORIGINAL poses and the
    accumulated offset, and reports it."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    CB = importlib.import_module("global-lvba_amd.calib")
    calls = []

    def fake6(records, table, poses, intr, R, t, starts=None, device=0, **opts):
        calls.append(("six", np.array(poses), opts))
        return R, t, dict(Rci=R, tci=t, status=0, iterations=1, n_used=5, rmse_px=0.1, cost=0.0, n_held=0, eigenvalues=np.ones(6),
                          eigenvectors=np.eye(6), information=np.eye(6))

    def fake7(records, table, poses, twists, intr, R, t, td0=0.0, starts=None, device=0, **opts):
        calls.append(("seven", np.array(poses), float(td0)))
        return R, t, td0 + 0.01, dict(Rci=R, tci=t, td=td0 + 0.01, status=0, iterations=1, n_used=5, rmse_px=0.1, cost=0.0, n_held=0,
                                      eigenvalues=np.ones(7), eigenvectors=np.eye(7), information=np.eye(7))

    lifted = []
    monkeypatch.setattr(CB, "refine_extrinsic", fake6)
    monkeypatch.setattr(CB, "refine_extrinsic_td", fake7)
    monkeypatch.setattr(CB, "linearize_td", lambda *a, **k: pytest.fail("a _td call on the default path"))
    monkeypatch.setattr(pl, "calibration_records", lambda kp, pairs, m, dk, Rcw, tcw, intr: lifted.append((Rcw, tcw)) or
                        (dict(pair=np.zeros(0, np.int32), uv=np.zeros((0, 2), np.float32), Xb=np.zeros((0, 3))), (np.zeros(0, np.int32),) * 2))

    class Depth:
        def close(self):
            pass

    case = tc.general()
    poses, tw = case["poses"], case["twists"]
    args = ([], [], [], poses, np.eye(3), np.zeros(3), np.ones(8))
    monkeypatch.setattr(CB, "refine_extrinsic_td", lambda *a, **k: pytest.fail("a _td call on the default path"))
    rep = pl.calibrate_extrinsic(*args, render=lambda R, t: Depth(), rounds=2)
    assert [c[0] for c in calls] == ["six", "six"] and rep["time_offset_s"] is None and "time_offset_rounds" not in rep
    monkeypatch.setattr(CB, "refine_extrinsic_td", fake7)
    del calls[:], lifted[:]
    rep = pl.calibrate_extrinsic(*args, render=lambda R, t: Depth(), rounds=2, time_offset=True, twists=tw)
    assert [(c[0], c[2]) for c in calls] == [("seven", 0.0), ("seven", 0.01)]
    for c in calls:
        np.testing.assert_array_equal(c[1], poses)                                # the solver gets the original poses
    want = pl.camera_from_imu(CB.shift_poses(poses, tw, 0.01), np.eye(3), np.zeros(3))
    np.testing.assert_array_equal(lifted[1][0], want[0])                          # the second round lifts at the shifted ones
    np.testing.assert_array_equal(lifted[1][1], want[1])
    np.testing.assert_array_equal(lifted[0][0], pl.camera_from_imu(poses, np.eye(3), np.zeros(3))[0])
    assert rep["time_offset_s"] == 0.02 and rep["time_offset_rounds"] == [0.01, 0.02]
    with pytest.raises(ValueError, match="twists"):
        pl.calibrate_extrinsic(*args, render=lambda R, t: Depth(), time_offset=True)


def test_run_full_pipeline_takes_the_twists_from_the_lidar_trajectory_and_hands_shifted_poses_on(monkeypatch):
    """time_offset in the keyword: the twists are body_twists of the refined scan poses at the image times; with apply and a
    converged result the visual stage gets the image poses shifted by the offset, and the report says so; without apply it does not."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    CB = importlib.import_module("global-lvba_amd.calib")

    class Depth:
        def close(self):
            pass

    scan_poses = np.zeros((3, 12))
    for k in range(3):
        scan_poses[k, :9], scan_poses[k, 9:] = co.rodrigues([0.0, 0.0, 0.05 * k]).reshape(9), [0.2 * k, 0.0, 0.0]
    scan_t, img_t = np.array([0.0, 0.1, 0.2]), np.array([0.05, 0.15])
    img_poses = scan_poses[:2].copy()
    seen, calls = [], []

    def fake(*a, **k):
        seen.append(k)
        return dict(status="converged", Rci=np.eye(3).tolist(), tci=[0.0, 0.0, 0.0], time_offset_s=0.02)

    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl.V.DepthImages, "render", staticmethod(lambda *a, **k: Depth()))
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append(a) or {})
    monkeypatch.setattr(pl, "_calibrate_extrinsic", fake)
    kps = [np.zeros((5, 2), np.float32)] * 2
    args = ([np.zeros((3, 3), np.float32)] * 3, scan_poses, scan_t, img_t, img_poses, np.eye(3), np.zeros(3), np.ones(8), 640, 512, kps, [(0, 1)],
            [np.array([[0, 1], [2, 3]], np.int32)])
    fn = lambda cams, depth=None: ([(0, 1)], [np.array([[0, 1]], np.int32)])
    out = pl.run_full_pipeline(*args, enable_lidar_ba=False, match_fn=fn, match_depth=True, calibrate_extrinsic=dict(time_offset=True))
    tw = pl.body_twists(scan_poses, scan_t, img_t)
    np.testing.assert_array_equal(seen[0]["twists"], tw)
    assert seen[0]["time_offset"] is True and out["extrinsic"]["applied"] is False and out["extrinsic"]["poses_shifted"] is False
    np.testing.assert_array_equal(calls[0][5], img_poses)                         # the image poses as they came
    out = pl.run_full_pipeline(*args, enable_lidar_ba=False, match_fn=fn, match_depth=True, calibrate_extrinsic=dict(time_offset=True, apply=True))
    assert out["extrinsic"]["applied"] is True and out["extrinsic"]["poses_shifted"] is True
    cam = pl.update_camera_poses_from_lidar(scan_poses, scan_poses, scan_t, img_t, img_poses)
    want = CB.shift_poses(cam, tw, 0.02)
    got = pl.update_camera_poses_from_lidar(calls[1][1], calls[1][2], scan_t, img_t, calls[1][5])   # what the visual stage derives
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert np.abs(want - cam).max() > 1e-3
    out = pl.run_full_pipeline(*args, enable_lidar_ba=False, match_fn=fn, match_depth=True, calibrate_extrinsic="apply")
    assert "poses_shifted" not in out["extrinsic"] and "twists" not in seen[2]
    np.testing.assert_array_equal(calls[2][5], img_poses)


def test_run_dataset_writes_the_offset_into_the_report(tmp_path, monkeypatch):
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
    report = dict(status="converged", n_used=200, n_held=0, Rci=np.eye(3).tolist(), tci=[0.0, 0.0, 0.0], applied=False, rounds=[],
                  time_offset_s=0.02, std_td_s=1e-4, time_offset_rounds=[0.02], poses_shifted=False)
    monkeypatch.setattr(pl, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict(extrinsic=report, poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    kw = dict(time_offset=True, rounds=2)
    pl.run_dataset(str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3), out_dir=str(tmp_path / "out"), calibrate_extrinsic=kw)
    assert calls[0]["calibrate_extrinsic"] == kw
    assert json.load(open(tmp_path / "out" / "extrinsic.json")) == report
