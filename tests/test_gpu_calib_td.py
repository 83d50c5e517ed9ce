"""GPU tests of the extrinsic refinement with a time offset (lvba_calib_*_td; include/lvba_hip.h, DESIGN.md §10o "time offset")
against the numpy oracle (tests/calib_td_oracle.py) on the seeded cases (tests/calib_td_cases.py).  A record's terms are the oracle's
bits, so every sum is held to the summation bound (n - 1) 2^-53 sum |term| at every edge of the kernel's partition; counts are
exact; the refined (R, t, td) is held to the truth where the records are exact and to the oracle's own run, within what the order
of summation changes, where they are noisy."""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

import calib_cases as cc
import calib_oracle as co
import calib_td_cases as tc
import calib_td_oracle as cto

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TD = 0.013


@pytest.fixture(scope="module")
def CB(pkg):
    return importlib.import_module("global-lvba_amd.calib")


def records_of(case, keep=None):
    keep = slice(None) if keep is None else keep
    return dict(pair=case["pair"][keep], uv=case["uv"][keep], Xb=case["Xb"][keep])


def table_of(case):
    return (case["img_a"], case["img_b"]), case["poses"], case["twists"], case["intr"]


def device_sums(CB, case, rec, R, t, td, **kw):
    """[J, NS] in the oracle's layout, from lvba_calib_linearize_td (sum rho' is not an output: left out of every comparison)"""
    H, g, cost, n_used, ssq = CB.linearize_td(rec, *table_of(case), R, t, td, **kw)
    J = len(cost)
    s = np.zeros((J, cto.NS))
    iu = np.triu_indices(7)
    for j in range(J):
        assert np.array_equal(H[j], H[j].T)
        s[j, :28] = H[j][iu]
        s[j, cto.G0:cto.G0 + 7] = g[j]
        s[j, cto.COST], s[j, cto.CNT], s[j, cto.SSQ] = cost[j], n_used[j], ssq[j]
    return s


def check_sums(got, want, abs_sum, n_counted, what):
    assert got[cto.CNT] == want[cto.CNT] == n_counted, what
    bound = max(n_counted - 1, 0) * U * abs_sum
    q = np.r_[0:cto.SW]                                                           # every sum the call returns
    worst = np.abs(got[q] - want[q]) - bound[q]
    assert (worst <= 0).all(), (what, np.argmax(worst), got[q][np.argmax(worst)], want[q][np.argmax(worst)], bound[q][np.argmax(worst)])


def oracle_terms(case, td=TD, **kw):
    E = cto.pair_table(case["poses"], case["twists"], case["img_a"], case["img_b"], td)
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    e = cto.evaluate(case["R0"], case["t0"], E, case["pair"], xy, case["Xb"], case["intr"], cto.options(**kw))
    return cto.terms(e), e["counted"]


def prefix_sums(T, sizes):
    out = np.zeros((len(sizes), len(T)))
    for q in range(len(T)):
        out[:, q] = np.concatenate([[0.0], np.cumsum(T[q])])[np.asarray(sizes, np.int64)]
    return out


@pytest.fixture(scope="module")
def wide_terms():
    """the terms of every record of the widest case at its planted extrinsic and td = 0.013, computed once"""
    h = tc.header_constants()
    cap = h["CAL_BLOCK"] * h["CAL_RUN"] * h["CAL_MAX_BLOCKS"]
    case = tc.wide(cap + 1)
    T, counted = oracle_terms(case)
    return case, T, counted


def test_linearize_at_every_edge_of_the_partition(CB, wide_terms):
    """0 and 1 record; one wavefront - 1 / exactly / + 1; one workgroup +- 1; one workgroup's full run +- 1; the cap on workgroups
    +- 1 record (the constants are the header's); at td = 0.013"""
    h = tc.header_constants()
    W, B = 64, h["CAL_BLOCK"]
    run = B * h["CAL_RUN"]
    cap = run * h["CAL_MAX_BLOCKS"]
    sizes = [0, 1, W - 1, W, W + 1, B - 1, B, B + 1, run - 1, run, run + 1, cap - 1, cap, cap + 1]
    case, T, counted = wide_terms
    assert len(case["pair"]) >= cap + 1 and counted[:cap + 1].all()
    want = prefix_sums(T, sizes)
    abs_sum = prefix_sums(np.abs(T), sizes)
    for k, n in enumerate(sizes):
        got = device_sums(CB, case, records_of(case, slice(0, n)), case["R0"], case["t0"], TD)[0]
        check_sums(got, want[k], abs_sum[k], n, n)
        if n <= 1:
            np.testing.assert_array_equal(got[:cto.SW], want[k][:cto.SW])         # nothing to reorder
        if n == 1:
            assert got[6] != 0.0                                                  # the seventh column is there


def test_unusable_and_behind_camera_records_at_lane_edges(CB):
    """at the first and the last lane of a wavefront and of a workgroup, of either workgroup of a two-workgroup grid, and on a lane's
    second record: not counted, and the sums are the oracle's without them"""
    h = tc.header_constants()
    B = h["CAL_BLOCK"]
    n = B * h["CAL_RUN"] + 2 * B                                                  # two workgroups
    base = tc.general()
    bad = np.array([0, 63, 64, 127, B - 1, B, 2 * B - 1, 2 * B, 2 * B + 63, n - 1])
    case = dict(base, uv=base["uv"][:n].copy(), Xb=base["Xb"][:n].copy(), pair=base["pair"][:n])
    for k, i in enumerate(bad):
        if k % 3 == 0:
            case["uv"][i] = np.nan
        elif k % 3 == 1:
            case["Xb"][i, k % 2] = np.inf if k % 2 else np.nan
        else:
            case["Xb"][i] *= -1.0                                                 # behind the camera
    T, counted = oracle_terms(case)
    keep = np.ones(n, bool)
    keep[bad] = False
    np.testing.assert_array_equal(counted, keep)
    want = cto.sums(T)
    np.testing.assert_array_equal(want, cto.sums(T[:, keep]))                     # the oracle without them: the same sums
    got = device_sums(CB, case, records_of(case), case["R0"], case["t0"], TD)[0]
    check_sums(got, want, np.abs(T).sum(axis=1), n - len(bad), "edges")


def job_bytes(rep, j):
    return b"".join(np.ascontiguousarray(rep[k][j]).tobytes() for k in sorted(rep))


def test_same_bytes_wherever_a_job_stands(CB):
    """a job alone, in a batch of three with different (R, t, td0), and in that batch reversed"""
    case = tc.noisy()
    args = (records_of(case), *table_of(case))
    starts = [(case["R0"], case["t0"], 0.0), (case["R_true"], case["t_true"], 0.05),
              co.perturb(case["R_true"], case["t_true"], np.r_[0.02, -0.01, 0.03, 0.05, 0.0, -0.04]) + (-0.03,)]
    R = np.array([s[0] for s in starts])
    t = np.array([s[1] for s in starts])
    td = np.array([s[2] for s in starts])
    three = CB.refine_jobs_td(*args, R, t, td)
    rev = CB.refine_jobs_td(*args, R[::-1].copy(), t[::-1].copy(), td[::-1].copy())
    print("iterations of the three jobs:", three["iterations"], "td", three["td"])
    assert (three["status"] == CB.CONVERGED).all()
    for j in range(3):
        alone = CB.refine_jobs_td(*args, R[j:j + 1], t[j:j + 1], td[j:j + 1])
        assert job_bytes(three, j) == job_bytes(alone, 0) == job_bytes(rev, 2 - j), j
    lin = [CB.linearize_td(*args, R, t, td) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*lin))
    Rb, tb, tdb, rep = CB.refine_extrinsic_td(*args, case["R0"], case["t0"], 0.0, starts=[(case["R_true"], case["t_true"]), starts[2]])
    assert (rep["jobs"]["status"] == CB.CONVERGED).all() and rep["job"] == int(np.argmin(rep["jobs"]["cost"])) and tdb == rep["jobs"]["td"][rep["job"]]


@pytest.mark.parametrize("td_true", [0.02, -0.05])
def test_recovers_the_planted_extrinsic_and_offset_on_the_general_trajectory(CB, td_true):
    """from 3 degrees / 10 cm / 0 s off: within 1e-9 rad, 1e-9 m (the project's bars) and 1e-9 s -- no tighter than those two: a
    second of offset moves a pixel by at most what |om| <= 0.5 rad plus |v| <= 1 m do.  Measured on the CPU by the oracle alone
    (tests/test_calib_td_host.py::test_held_sets_and_recovery): 4.2e-13 rad, 2.0e-12 m, 1.7e-14 s at 0.02 and 4.8e-12 rad, 1.7e-11 m,
    1.3e-12 s at -0.05.  Measured on the device: 4.2e-13 rad, 2.0e-12 m, 1.7e-14 s and 4.8e-12 rad, 1.7e-11 m, 1.3e-12 s, three steps
    each."""
    case = tc.general(td_true)
    R, t, td, rep = CB.refine_extrinsic_td(records_of(case), *table_of(case), case["R0"], case["t0"])
    d = co.left_difference(R, t, case["R_true"], case["t_true"])
    print("general", td_true, ": iterations", rep["iterations"], "rmse", rep["rmse_px"], "error", np.linalg.norm(d[:3]), "rad", np.linalg.norm(d[3:]),
          "m", abs(td - td_true), "s")
    assert rep["status"] == CB.CONVERGED and rep["n_held"] == 0 and rep["n_used"] == len(case["pair"])
    assert np.linalg.norm(d[:3]) <= 1e-9 and np.linalg.norm(d[3:]) <= 1e-9 and abs(td - td_true) <= 1e-9
    assert np.array_equal(rep["information"], rep["information"].T) and (np.diff(rep["eigenvalues"]) >= 0).all()
    V, lam = rep["eigenvectors"], rep["eigenvalues"]
    assert np.abs(V @ rep["information"] @ V.T - np.diag(lam)).max() <= 1e-12 * lam.max()
    s = CB.summary(rep, case["R0"], case["t0"])
    assert s["time_offset_s"] == td and s["std_td_s"] is not None and s["held"] == []


def test_planar_holds_the_translation_along_the_axis_and_recovers_the_offset(CB):
    case = tc.planar()
    R, t, td, rep = CB.refine_extrinsic_td(records_of(case), *table_of(case), case["R0"], case["t0"])
    assert rep["status"] == CB.CONVERGED and rep["n_held"] == 1
    want = np.r_[cc.held_span("planar", R, t)[0], 0.0]
    assert cc.principal_angles(want[None], rep["eigenvectors"][:1]).max() < 1e-6
    Rt = case["R_true"].reshape(3, 3)
    Zr = co.left_difference(Rt.T @ R, np.zeros(3), np.eye(3), np.zeros(3))[:3]
    Zt = Rt.T @ (t - case["t_true"])
    print("planar: free error", np.linalg.norm(Zr), np.linalg.norm(Zt[:2]), abs(td - case["td_true"]), "held part", Zt[2])
    assert np.linalg.norm(Zr) <= 1e-9 and np.linalg.norm(Zt[:2]) <= 1e-9 and abs(td - case["td_true"]) <= 1e-9


def test_noise_and_outliers_against_the_oracles_own_run(CB):
    """0.5 px, 20 % gross outliers, Huber at 2 px: the device's (R, t, td) against the oracle's run of the same rule with its sums in
    index order, within 16 times what the order of summation changes there (calib_td_cases.NOISY_TOL = 7.2e-15, measured on the
    CPU).  Measured on the device: 4.4e-16 in R, 2.9e-16 in t, 3.1e-17 in td, the same five steps."""
    case = tc.noisy()
    R, t, td, rep = CB.refine_extrinsic_td(records_of(case), *table_of(case), case["R0"], case["t0"])
    want = cto.solve(case["poses"], case["twists"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"],
                     case["R0"], case["t0"])
    dR, dt, dtd = np.abs(R.reshape(9) - want["R"]).max(), np.abs(t - want["t"]).max(), abs(td - want["td"])
    print("noisy: device against oracle: R", dR, "t", dt, "td", dtd, "allowed", tc.NOISY_TOL, "; iterations", rep["iterations"], want["iterations"])
    assert rep["status"] == CB.CONVERGED == want["status"] and rep["iterations"] == want["iterations"] and rep["n_held"] == 0
    assert rep["n_used"] == want["n_used"] and abs(rep["rmse_px"] - want["rmse_px"]) <= 1e-12 * want["rmse_px"]
    assert dR <= tc.NOISY_TOL and dt <= tc.NOISY_TOL and dtd <= tc.NOISY_TOL


def test_constant_twist_holds_the_offset(CB):
    case = tc.screw()
    for td0 in (0.0, 0.01):
        R, t, td, rep = CB.refine_extrinsic_td(records_of(case), *table_of(case), case["R0"], case["t0"], td0)
        assert rep["status"] == CB.CONVERGED and rep["n_held"] == 3 and abs(td - td0) <= 1e-12
        assert cc.principal_angles(tc.screw_held_span(case, R, t), rep["eigenvectors"][:3]).max() < 1e-6


def test_zero_twists_return_the_six_parameter_bytes(CB):
    case = tc.zero()
    six = CB.refine_jobs(records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"], case["R0"], case["t0"])
    for td0 in (0.0, 0.04):
        seven = CB.refine_jobs_td(records_of(case), *table_of(case), case["R0"], case["t0"], td0)
        for k in ("Rci", "tci", "status", "iterations", "n_used", "rmse_px", "cost"):
            assert seven[k].tobytes() == six[k].tobytes(), k
        assert seven["td"][0] == td0 and seven["n_held"][0] == six["n_held"][0] + 1 and six["status"][0] == CB.CONVERGED
        assert seven["information"][0][:6, :6].tobytes() == six["information"][0].tobytes() and not seven["information"][0][6].any()


def test_status_paths(CB):
    case = tc.general()
    tab = table_of(case)
    few = CB.refine_jobs_td(records_of(case, slice(0, 99)), *tab, case["R0"], case["t0"], 0.01)
    assert few["status"][0] == CB.TOO_FEW_RECORDS and few["n_used"][0] == 99 and few["iterations"][0] == 0 and few["td"][0] == 0.01
    np.testing.assert_array_equal(few["Rci"][0].reshape(9), case["R0"])
    none = CB.refine_jobs_td(records_of(case, slice(0, 0)), *tab, case["R0"], case["t0"], min_records=0)
    assert none["status"][0] == CB.DEGENERATE and none["n_held"][0] == 7 and none["n_used"][0] == 0
    still = (tab[0], np.tile(case["poses"][3], (len(case["poses"]), 1)), np.zeros_like(case["twists"]), tab[3])
    deg = CB.refine_jobs_td(records_of(case), *still, case["R0"], case["t0"])
    assert deg["status"][0] == CB.DEGENERATE and deg["n_held"][0] == 7 and deg["iterations"][0] == 0
    one = CB.refine_jobs_td(records_of(case), *tab, case["R0"], case["t0"], max_iterations=1)
    assert one["status"][0] == CB.MAX_ITERATIONS and one["iterations"][0] == 1 and one["td"][0] != 0.0
    H, g, cost, n_used, ssq = CB.linearize_td(records_of(case), *tab, one["Rci"], one["tci"], one["td"])
    assert H[0].tobytes() == one["information"][0].tobytes() and cost[0] == one["cost"][0]      # of what it returns
    far = tc.general(0.3)                                                          # past the default bound of 0.2 s
    out = CB.refine_jobs_td(records_of(far), *table_of(far), far["R0"], far["t0"], 0.01)
    assert out["status"][0] == CB.TD_OUT_OF_RANGE and out["td"][0] == 0.01
    np.testing.assert_array_equal(out["Rci"][0].reshape(9), far["R0"])
    np.testing.assert_array_equal(out["tci"][0], far["t0"])
    ok = CB.refine_jobs_td(records_of(far), *table_of(far), far["R0"], far["t0"], max_abs_td_s=0.5)
    assert ok["status"][0] == CB.CONVERGED and abs(ok["td"][0] - 0.3) <= 1e-9
    o = CB.calib_td_opts()
    assert (o.eps_td_s, o.max_abs_td_s, o.calib.max_iterations, o.calib.loss_kind, o.calib.min_eig_ratio) == (1e-10, 0.2, 20, 1, 1e-6)
    assert C.sizeof(CB.L.CalibTdOpts) == 88 and CB.calib_td_opts(loss_kind="cauchy", eps_td_s=1e-6).calib.loss_kind == 3
    assert CB.L.load().lvba_version() == 112


def raw_call(CB, case, which, o=None, **mod):
    """the C call with every output filled beforehand: (status, untouched)"""
    lib = CB.L.load()
    a = dict(poses=np.ascontiguousarray(case["poses"]), twists=np.ascontiguousarray(case["twists"]), intr=np.ascontiguousarray(case["intr"]),
             img_a=case["img_a"].copy(), img_b=case["img_b"].copy(), pair=case["pair"].copy(), uv=case["uv"].copy(), Xb=case["Xb"].copy(),
             R=case["R0"].copy(), t=case["t0"].copy(), td=np.array([0.01]), M=len(case["poses"]), n_jobs=1)
    a.update(mod)
    p = lambda k: None if a[k] is None else a[k].ctypes.data
    o = CB.calib_td_opts() if o is None else o
    head = (0, a["M"], p("poses"), p("twists"), p("intr"), len(a["img_a"]), p("img_a"), p("img_b"), len(a["pair"]), p("pair"), p("uv"), p("Xb"),
            a["n_jobs"], p("R"), p("t"), p("td"), C.byref(o))
    if which == "extrinsic":
        outs = [np.full(9, -7.0), np.full(3, -7.0), np.full(1, -7.0), np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7, np.int64),
                np.full(1, -7.0), np.full(1, -7.0), np.full(1, -7, np.int32), np.full(7, -7.0), np.full(49, -7.0), np.full(49, -7.0)]
        rc = lib.lvba_calib_extrinsic_td(*head, *[x.ctypes.data for x in outs])
    else:
        outs = [np.full(49, -7.0), np.full(7, -7.0), np.full(1, -7.0), np.full(1, -7, np.int64), np.full(1, -7.0)]
        rc = lib.lvba_calib_linearize_td(*head, *[x.ctypes.data for x in outs])
    return rc, all((x == -7).all() for x in outs)


def _with(a, i, v):
    a = a.copy()
    a.reshape(-1)[i] = v
    return a


def test_every_argument_error_writes_nothing(CB):
    L = CB.L
    base = tc.general()
    case = dict(base, pair=base["pair"][:2000], uv=base["uv"][:2000], Xb=base["Xb"][:2000])
    bad = lambda k, i, v: {k: _with(np.ascontiguousarray(case[{"R": "R0", "t": "t0"}.get(k, k)]), i, v)}
    split = case["pair"].copy()
    split[10] = 3                                                                 # pair 0, 3, 0, ...: not one run per pair
    mods = [dict(poses=None), dict(intr=None), dict(R=None), dict(uv=None), dict(M=0), dict(n_jobs=0),
            bad("pair", 5, len(case["img_a"])), bad("pair", 5, -1), dict(pair=split),
            bad("img_a", 2, len(case["poses"])), bad("img_b", 2, -1), bad("img_a", 4, int(case["img_b"][4])),
            bad("poses", 17, np.nan), bad("intr", 5, np.inf), bad("R", 4, np.nan), bad("t", 1, np.inf), bad("intr", 0, 0.0), bad("intr", 1, -600.0),
            # the time offset's own
            dict(twists=None), bad("twists", 7, np.nan), bad("twists", 58, np.inf), dict(td=None), dict(td=np.array([np.nan])),
            dict(td=np.array([np.inf])), dict(td=np.array([0.21])), dict(td=np.array([-0.21]))]
    for which in ("extrinsic", "linearize"):
        assert raw_call(CB, case, which)[0] == L.OK
        for m in mods:
            rc, untouched = raw_call(CB, case, which, **m)
            assert rc == L.ERR_ARG and untouched, (which, list(m))
        for kw in (dict(max_iterations=0), dict(max_error_px=-1.0), dict(min_eig_ratio=-1e-9), dict(eps_rot=-1.0), dict(eps_trans=-1.0),
                   dict(min_records=-1), dict(loss_scale_px=-2.0), dict(loss_kind=9), dict(eps_rot=np.nan),
                   dict(eps_td_s=-1e-12), dict(eps_td_s=np.nan), dict(max_abs_td_s=0.0), dict(max_abs_td_s=-1.0), dict(max_abs_td_s=np.nan)):
            rc, untouched = raw_call(CB, case, which, o=CB.calib_td_opts(**kw))
            assert rc == L.ERR_ARG and untouched, (which, kw)
        assert raw_call(CB, case, which, td=np.array([0.21]), o=CB.calib_td_opts(max_abs_td_s=0.25))[0] == L.OK
    with pytest.raises(TypeError):
        CB.calib_td_opts(hypotheses=3)
    with pytest.raises(L.LvbaError) as e:
        CB.refine_jobs_td(records_of(case), *table_of(case), case["R0"], case["t0"], 0.5)
    assert e.value.code == L.ERR_ARG
    assert raw_call(CB, case, "extrinsic")[0] == L.OK                             # and the library is usable afterwards


def test_pipeline_recovers_a_planted_offset_on_the_room_sequence(CB, pkg):
    """calib_td_cases.room_sequence: scans at the given poses, images taken 30 ms later under seeded twists of up to 0.5 rad/s and
    1 m/s.  calibrate_extrinsic(time_offset=True, rounds=2) from 2 degrees and 10.8 cm off: the offset ends nearer the truth than
    zero, with the right sign, and the extrinsic ends nearer the planted one than the 6-parameter call's on the same sequence."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    V = importlib.import_module("global-lvba_amd.visual")
    voxel = importlib.import_module("global-lvba_amd.voxel")
    d = tc.room_sequence()
    R0, t0 = co.perturb(cc.ROOM_RCI.reshape(9), cc.ROOM_TCI, cc.ROOM_PLANT)
    c = pipe.DEFAULTS
    err = {}
    with voxel.Scans(d["clouds"]) as scans:
        render = lambda Rk, tk: V.DepthImages.render(scans, d["poses"], d["times"], d["times"], Rk, tk, cc.ROOM_INTR, cc.ROOM_W, cc.ROOM_H,
                                                     half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
        for on in (False, True):
            rep = pipe.calibrate_extrinsic(d["kps"], d["pairs"], d["matches"], d["poses"], R0.reshape(3, 3), t0, cc.ROOM_INTR, render=render,
                                           rounds=2, **(dict(time_offset=True, twists=d["twists"]) if on else {}))
            e = co.left_difference(np.array(rep["Rci"]), np.array(rep["tci"]), cc.ROOM_RCI, cc.ROOM_TCI)
            err[on] = (np.linalg.norm(e[:3]), np.linalg.norm(e[3:]))
            print("time_offset", on, rep["status"], "n_held", rep["n_held"], "records", rep["n_records"], "rmse %.3f px" % rep["rmse_px"],
                  "error %.5f deg %.5f m" % (np.degrees(err[on][0]), err[on][1]), "td", rep["time_offset_s"], "std", rep["std_td_s"],
                  rep.get("time_offset_rounds"))
            # (the 6-parameter rule, which has no way to explain the offset, may still be moving at its iteration limit)
            assert rep["status"] in (("converged",) if on else ("converged", "max_iterations")) and len(rep["rounds"]) == 2
            json.dumps(rep)
            if on:
                assert abs(rep["time_offset_s"] - d["td_true"]) < 0.015 and rep["time_offset_s"] > 0.0
                assert len(rep["time_offset_rounds"]) == 2 and rep["time_offset_rounds"][1] == rep["time_offset_s"] and rep["std_td_s"] > 0.0
            else:
                assert rep["time_offset_s"] is None and "time_offset_rounds" not in rep
    assert err[True][0] < err[False][0] and err[True][1] < err[False][1]


def test_run_full_pipeline_and_run_dataset_carry_the_keyword(CB, pkg, tmp_path, monkeypatch):
    """run_full_pipeline(calibrate_extrinsic=dict(time_offset=True)) takes the twists from the refined LiDAR trajectory and reports
    the offset; with apply the report says whether the image poses were shifted; run_dataset writes the keys into extrinsic.json."""
    import test_gpu_mapq as tm
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = tm._dataset()
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    odo = d["odo"]
    args = (d["clouds"], odo, d["times"], d["img_t"], odo, tm.RCB, tm.TCI, tm.INTR, tm.W, tm.H, d["kps"], d["pairs"], d["matches"])
    on = pipe.run_full_pipeline(*args, enable_lidar_ba=False, calibrate_extrinsic=dict(time_offset=True, max_iterations=5),
                                **cfg)
    rep = on["extrinsic"]
    print("loop sequence:", rep["status"], "td", rep["time_offset_s"], "std", rep["std_td_s"], "n_held", rep["n_held"])
    assert isinstance(rep["time_offset_s"], float) and rep["applied"] is False and rep["poses_shifted"] is False
    assert len(rep["time_offset_rounds"]) <= 1 and len(rep["eigenvalues"]) == 7
    # run_dataset hands the keyword on and writes that report, new keys included, into extrinsic.json (a two-image stand-in
    # dataset; the pipeline's answer is the report above)
    import sqlite3
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
    monkeypatch.setattr(pipe, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict(extrinsic=rep, poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    kw = dict(time_offset=True, max_iterations=5)
    pipe.run_dataset(str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3), out_dir=str(tmp_path / "out"), calibrate_extrinsic=kw)
    assert calls[0]["calibrate_extrinsic"] == kw
    written = json.load(open(tmp_path / "out" / "extrinsic.json"))
    assert written == rep and {"time_offset_s", "std_td_s", "time_offset_rounds", "poses_shifted"} <= set(written)
