"""GPU tests of the extrinsic refinement (lvba_calib_*; include/lvba_hip.h) against the numpy oracle
(tests/calib_oracle.py) on the seeded cases (tests/calib_cases.py).  A record's terms are the oracle's bits, so every sum is held to
the summation bound (n - 1) 2^-53 sum |term| at every edge of the kernel's partition; counts are exact; the refined extrinsic is held
to the planted one where the records are exact and to the oracle's own run, within what the order of summation changes, where they
are noisy."""
import ctypes as C
import importlib

import numpy as np
import pytest

import calib_cases as cc
import calib_oracle as co

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def CB(pkg):
    return importlib.import_module("global-lvba_amd.calib")


def records_of(case, keep=None):
    keep = slice(None) if keep is None else keep
    return dict(pair=case["pair"][keep], uv=case["uv"][keep], Xb=case["Xb"][keep])


def device_sums(CB, case, rec, R, t, **kw):
    """[J, NS] in the oracle's layout, from lvba_calib_linearize (sum rho' is not an output: left out of every comparison)"""
    H, g, cost, n_used, ssq = CB.linearize(rec, (case["img_a"], case["img_b"]), case["poses"], case["intr"], R, t, **kw)
    J = len(cost)
    s = np.zeros((J, co.NS))
    iu = np.triu_indices(6)
    for j in range(J):
        assert np.array_equal(H[j], H[j].T)
        s[j, :21] = H[j][iu]
        s[j, co.G0:co.G0 + 6] = g[j]
        s[j, co.COST], s[j, co.CNT], s[j, co.SSQ] = cost[j], n_used[j], ssq[j]
    return s


def check_sums(got, want, abs_sum, n_counted, what):
    assert got[co.CNT] == want[co.CNT] == n_counted, what
    bound = max(n_counted - 1, 0) * U * abs_sum
    q = np.r_[0:co.SW]                                                            # every sum the call returns
    worst = np.abs(got[q] - want[q]) - bound[q]
    assert (worst <= 0).all(), (what, np.argmax(worst), got[q][np.argmax(worst)], want[q][np.argmax(worst)], bound[q][np.argmax(worst)])


@pytest.fixture(scope="module")
def wide_terms():
    """the terms of every record of the widest case at its planted extrinsic, computed once: (case, T [NS, n], counted)"""
    h = cc.header_constants()
    cap = h["CAL_BLOCK"] * h["CAL_RUN"] * h["CAL_MAX_BLOCKS"]
    case = cc.wide(cap + 1)
    A = co.pair_transforms(case["poses"], case["img_a"], case["img_b"])
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    e = co.evaluate(case["R0"], case["t0"], A, case["pair"], xy, case["Xb"], case["intr"], co.options())
    return case, co.terms(e), e["counted"]


def test_linearize_at_every_edge_of_the_partition(CB, wide_terms):
    """0 and 1 record; one wavefront - 1 / exactly / + 1; one workgroup +- 1; one workgroup's full run +- 1; the cap on workgroups
    +- 1 record (the constants are the header's)."""
    h = cc.header_constants()
    W, B = 64, h["CAL_BLOCK"]
    run = B * h["CAL_RUN"]
    cap = run * h["CAL_MAX_BLOCKS"]
    sizes = [0, 1, W - 1, W, W + 1, B - 1, B, B + 1, run - 1, run, run + 1, cap - 1, cap, cap + 1]
    case, T, counted = wide_terms
    assert len(case["pair"]) >= cap + 1 and counted[:cap + 1].all()
    want = co.sums(T, prefixes=sizes)
    abs_sum = co.sums(np.abs(T), prefixes=sizes)
    for k, n in enumerate(sizes):
        got = device_sums(CB, case, records_of(case, slice(0, n)), case["R0"], case["t0"])[0]
        check_sums(got, want[k], abs_sum[k], n, n)
        if n <= 1:
            np.testing.assert_array_equal(got[:co.SW], want[k][:co.SW])           # nothing to reorder


def test_unusable_and_behind_camera_records_at_lane_edges(CB):
    """at the first and the last lane of a wavefront and of a workgroup, of either workgroup of a two-workgroup grid, and on a lane's
    second record: not counted, and the sums are the oracle's without them"""
    h = cc.header_constants()
    B = h["CAL_BLOCK"]
    n = B * h["CAL_RUN"] + 2 * B                                                 # two workgroups
    base = cc.general()
    bad = np.array([0, 63, 64, 127, B - 1, B, 2 * B - 1, 2 * B, 2 * B + 63, n - 1])
    case = dict(base, uv=base["uv"][:n].copy(), Xb=base["Xb"][:n].copy(), pair=base["pair"][:n])
    for k, i in enumerate(bad):
        if k % 3 == 0:
            case["uv"][i] = np.nan
        elif k % 3 == 1:
            case["Xb"][i, k % 2] = np.inf if k % 2 else np.nan
        else:
            case["Xb"][i] *= -1.0                                                # behind the camera
    A = co.pair_transforms(case["poses"], case["img_a"], case["img_b"])
    xy = co.targets(case["intr"], case["uv"], case["Xb"])
    e = co.evaluate(case["R0"], case["t0"], A, case["pair"], xy, case["Xb"], case["intr"], co.options())
    keep = np.ones(n, bool)
    keep[bad] = False
    np.testing.assert_array_equal(e["counted"], keep)
    T = co.terms(e)
    want = co.sums(T)
    np.testing.assert_array_equal(want, co.sums(T[:, keep]))                      # the oracle without them: the same sums
    got = device_sums(CB, case, records_of(case), case["R0"], case["t0"])[0]
    check_sums(got, want, np.abs(T).sum(axis=1), n - len(bad), "edges")


def test_gate_cuts_exactly_at_a_lane_boundary(CB):
    """the first three wavefronts' records pass the gate (set just above the largest error among them), every later record
    fails it: the count is 192 and the sums are the oracle's"""
    base = cc.general()
    A = co.pair_transforms(base["poses"], base["img_a"], base["img_b"])
    xy = co.targets(base["intr"], base["uv"], base["Xb"])
    s = co.evaluate(base["R0"], base["t0"], A, base["pair"], xy, base["Xb"], base["intr"], co.options())["s"]
    half = len(base["img_a"]) // 2
    med = np.median(s)
    inside = np.flatnonzero((s <= med) & (base["pair"] < half))[:192]           # index order: every pair's records in one run
    outside = np.flatnonzero((s > med * 1.01) & (base["pair"] >= half))[:300]
    order = np.r_[inside, outside]
    gate = float(np.sqrt(s[order[:192]].max()) * (1 + 1e-12))
    assert len(order) == 492 and (s[order[:192]] <= gate * gate).all() and (s[order[192:]] > gate * gate).all()
    case = dict(base, pair=base["pair"][order], uv=base["uv"][order], Xb=base["Xb"][order])
    o = co.options(max_error_px=gate)
    e = co.evaluate(case["R0"], case["t0"], A, case["pair"], xy[order], case["Xb"], case["intr"], o)
    assert e["counted"][:192].all() and not e["counted"][192:].any()
    T = co.terms(e)
    got = device_sums(CB, case, records_of(case), case["R0"], case["t0"], max_error_px=gate)[0]
    check_sums(got, co.sums(T), np.abs(T).sum(axis=1), 192, "gate")
    open_ = device_sums(CB, case, records_of(case), case["R0"], case["t0"])[0]
    assert open_[co.CNT] == 492


def job_bytes(rep, j):
    return b"".join(np.ascontiguousarray(rep[k][j]).tobytes() for k in sorted(rep))


def test_same_bytes_twice_and_wherever_a_job_stands(CB):
    case = cc.noisy()
    args = (records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"])
    starts = [(case["R0"], case["t0"]), (case["R_true"], case["t_true"]),
              co.perturb(case["R_true"], case["t_true"], np.r_[0.02, -0.01, 0.03, 0.05, 0.0, -0.04])]
    R = np.array([s[0] for s in starts])
    t = np.array([s[1] for s in starts])
    three = CB.refine_jobs(*args, R, t)
    again = CB.refine_jobs(*args, R, t)
    rev = CB.refine_jobs(*args, R[::-1].copy(), t[::-1].copy())
    print("iterations of the three jobs:", three["iterations"])                   # in lock-step, whenever each of them finishes
    assert (three["status"] == CB.CONVERGED).all()
    for j in range(3):
        alone = CB.refine_jobs(*args, R[j:j + 1], t[j:j + 1])
        assert job_bytes(three, j) == job_bytes(again, j) == job_bytes(alone, 0) == job_bytes(rev, 2 - j), j
    lin = [CB.linearize(*args, R, t) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*lin))
    # multi-start: the converged job of lowest cost, the lowest index of a tie
    Rb, tb, rep = CB.refine_extrinsic(*args, case["R0"], case["t0"], starts=starts[1:] + starts[:1])
    assert (rep["jobs"]["status"] == CB.CONVERGED).all() and rep["job"] == int(np.argmin(rep["jobs"]["cost"]))   # argmin: the first of a tie
    same = CB.refine_extrinsic(*args, case["R0"], case["t0"], starts=[(case["R0"], case["t0"])])[2]
    assert same["job"] == 0 and job_bytes(same["jobs"], 0) == job_bytes(same["jobs"], 1)


def test_recovers_the_planted_extrinsic_on_the_general_trajectory(CB):
    case = cc.general()
    R, t, rep = CB.refine_extrinsic(records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"], case["R0"], case["t0"])
    d = co.left_difference(R, t, case["R_true"], case["t_true"])
    print("general: iterations", rep["iterations"], "rmse", rep["rmse_px"], "error", np.linalg.norm(d[:3]), "rad", np.linalg.norm(d[3:]), "m")
    assert rep["status"] == CB.CONVERGED and rep["n_held"] == 0 and rep["n_used"] == len(case["pair"])
    assert np.linalg.norm(d[:3]) <= 1e-9 and np.linalg.norm(d[3:]) <= 1e-9
    assert np.array_equal(rep["information"], rep["information"].T) and (np.diff(rep["eigenvalues"]) >= 0).all()
    V, lam = rep["eigenvectors"], rep["eigenvalues"]
    assert np.abs(V @ rep["information"] @ V.T - np.diag(lam)).max() <= 1e-12 * lam.max()
    s = CB.summary(rep, case["R0"], case["t0"])
    assert abs(s["rotation_deg"] - cc.PLANT_ROT_DEG) < 1e-6 and abs(s["translation_m"] - cc.PLANT_TRANS) < 1e-6 and s["held"] == []


@pytest.mark.parametrize("name,n_held", [("screw", 2), ("planar", 1)])
def test_holds_what_a_single_axis_trajectory_leaves_unobservable(CB, name, n_held):
    """Screw (the body turns about one axis and moves along it): CONVERGED with n_held = 2, the held span is the oracle's and the
    theory's, the error in the free span is recovered (the result is the planted extrinsic times a member of the unobservable
    family), and the held components stay where they started.  Planar (a ground vehicle, which moves across its axis): one held."""
    case = getattr(cc, name)()
    R, t, rep = CB.refine_extrinsic(records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"], case["R0"], case["t0"])
    want = co.solve(case["poses"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"], case["R0"], case["t0"])
    assert rep["status"] == CB.CONVERGED == want["status"] and rep["n_held"] == n_held == want["n_held"]
    held = rep["eigenvectors"][:n_held]
    assert cc.principal_angles(want["vec"][:n_held], held).max() < 1e-6
    assert cc.principal_angles(cc.held_span(name, R, t), held).max() < 1e-6
    Rt, tt = case["R_true"].reshape(3, 3), case["t_true"]
    Zr = co.left_difference(Rt.T @ R, np.zeros(3), np.eye(3), np.zeros(3))[:3]   # X*^-1 X: a turn about z and a shift along it at most
    Zt = Rt.T @ (t - tt)
    free = np.r_[Zr[:2] if n_held == 2 else Zr, Zt[:2]]
    print(name, "free error", free, "held part", Zr[2], Zt[2])
    assert np.linalg.norm(free[:-2]) <= 1e-9 and np.linalg.norm(free[-2:]) <= 1e-9
    d0 = co.left_difference(R, t, case["R0"], case["t0"])
    assert np.abs(held @ d0).max() <= d0 @ d0                                    # second order in the distance moved at most
    w0 = co.left_difference(want["R"], want["t"], case["R0"], case["t0"])           # the oracle's run moved as far along the held span
    assert abs(np.linalg.norm(held @ d0) - np.linalg.norm(want["vec"][:n_held] @ w0)) <= 1e-6 * np.linalg.norm(d0) + 1e-9


def test_noise_and_outliers_against_the_oracles_own_run(CB):
    """0.5 px, 20 % gross outliers, Huber at 2 px: the device's extrinsic against the oracle's run of the same rule with its sums
    in index order, within 16 times what the order of summation changes there (calib_cases.NOISY_TOL, measured on the CPU)."""
    case = cc.noisy()
    R, t, rep = CB.refine_extrinsic(records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"], case["R0"], case["t0"])
    want = co.solve(case["poses"], case["img_a"], case["img_b"], case["pair"], case["uv"], case["Xb"], case["intr"], case["R0"], case["t0"])
    dR, dt = np.abs(R.reshape(9) - want["R"]).max(), np.abs(t - want["t"]).max()
    print("noisy: device against oracle: R", dR, "t", dt, "allowed", cc.NOISY_TOL, "; iterations", rep["iterations"], want["iterations"])
    assert rep["status"] == CB.CONVERGED == want["status"] and rep["iterations"] == want["iterations"] and rep["n_held"] == 0
    assert rep["n_used"] == want["n_used"] and abs(rep["rmse_px"] - want["rmse_px"]) <= 1e-12 * want["rmse_px"]
    assert dR <= cc.NOISY_TOL and dt <= cc.NOISY_TOL


def test_status_paths(CB):
    case = cc.general()
    table, poses, intr = (case["img_a"], case["img_b"]), case["poses"], case["intr"]
    few = CB.refine_jobs(records_of(case, slice(0, 99)), table, poses, intr, case["R0"], case["t0"])
    assert few["status"][0] == CB.TOO_FEW_RECORDS and few["n_used"][0] == 99 and few["iterations"][0] == 0
    np.testing.assert_array_equal(few["Rci"][0].reshape(9), case["R0"])           # the extrinsic comes back as it went in
    assert CB.refine_jobs(records_of(case, slice(0, 100)), table, poses, intr, case["R0"], case["t0"])["status"][0] != CB.TOO_FEW_RECORDS
    none = CB.refine_jobs(records_of(case, slice(0, 0)), table, poses, intr, case["R0"], case["t0"], min_records=0)
    assert none["status"][0] == CB.DEGENERATE and none["n_held"][0] == 6 and none["n_used"][0] == 0
    still = np.tile(poses[3], (len(poses), 1))                                   # the body never moves: nothing is observable
    deg = CB.refine_jobs(records_of(case), table, still, intr, case["R0"], case["t0"])
    assert deg["status"][0] == CB.DEGENERATE and deg["n_held"][0] == 6 and deg["iterations"][0] == 0
    np.testing.assert_array_equal(deg["tci"][0], case["t0"])
    one = CB.refine_jobs(records_of(case), table, poses, intr, case["R0"], case["t0"], max_iterations=1)
    assert one["status"][0] == CB.MAX_ITERATIONS and one["iterations"][0] == 1
    # what a job reports is of the extrinsic it returns
    H, g, cost, n_used, ssq = CB.linearize(records_of(case), table, poses, intr, one["Rci"], one["tci"])
    assert H[0].tobytes() == one["information"][0].tobytes() and cost[0] == one["cost"][0]
    o = CB.calib_opts()
    assert (o.max_iterations, o.loss_kind, o.min_records, o.loss_scale_px, o.max_error_px, o.min_eig_ratio, o.eps_rot, o.eps_trans) == \
        (20, 1, 100, 2.0, 0.0, 1e-6, 1e-10, 1e-10)
    assert C.sizeof(pkg_lib(CB).CalibOpts) == 64 and CB.calib_opts(loss_kind="cauchy").loss_kind == 3


def pkg_lib(CB):
    return CB.L


def raw_call(CB, case, which, o=None, **mod):
    """the C call with every output filled beforehand: (status, untouched)"""
    L = CB.L
    lib = L.load()
    a = dict(poses=np.ascontiguousarray(case["poses"]), intr=np.ascontiguousarray(case["intr"]), img_a=case["img_a"].copy(),
             img_b=case["img_b"].copy(), pair=case["pair"].copy(), uv=case["uv"].copy(), Xb=case["Xb"].copy(), R=case["R0"].copy(),
             t=case["t0"].copy(), M=len(case["poses"]), n_jobs=1)
    a.update(mod)
    p = lambda k: None if a[k] is None else a[k].ctypes.data
    o = CB.calib_opts() if o is None else o
    head = (0, a["M"], p("poses"), p("intr"), len(a["img_a"]), p("img_a"), p("img_b"), len(a["pair"]), p("pair"), p("uv"), p("Xb"), a["n_jobs"],
            p("R"), p("t"), C.byref(o))
    if which == "extrinsic":
        outs = [np.full(9, -7.0), np.full(3, -7.0), np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7, np.int64),
                np.full(1, -7.0), np.full(1, -7.0), np.full(1, -7, np.int32), np.full(6, -7.0), np.full(36, -7.0), np.full(36, -7.0)]
        rc = lib.lvba_calib_extrinsic(*head, *[x.ctypes.data for x in outs])
    else:
        outs = [np.full(36, -7.0), np.full(6, -7.0), np.full(1, -7.0), np.full(1, -7, np.int64), np.full(1, -7.0)]
        rc = lib.lvba_calib_linearize(*head, *[x.ctypes.data for x in outs])
    return rc, all((x == -7).all() for x in outs)


def test_every_argument_error_writes_nothing(CB):
    L = CB.L
    base = cc.general()
    case = dict(base, pair=base["pair"][:2000], uv=base["uv"][:2000], Xb=base["Xb"][:2000])
    bad = lambda k, i, v: {k: _with(np.ascontiguousarray(case[{"R": "R0", "t": "t0"}.get(k, k)]), i, v)}
    split = case["pair"].copy()
    split[10] = 3                                                                 # pair 0, 3, 0, ...: not one run per pair
    mods = [dict(poses=None), dict(intr=None), dict(R=None), dict(uv=None), dict(M=0), dict(n_jobs=0),
            bad("pair", 5, len(case["img_a"])), bad("pair", 5, -1), dict(pair=split),
            bad("img_a", 2, len(case["poses"])), bad("img_b", 2, -1), bad("img_a", 4, int(case["img_b"][4])),
            bad("poses", 17, np.nan), bad("intr", 5, np.inf), bad("R", 4, np.nan), bad("t", 1, np.inf), bad("intr", 0, 0.0), bad("intr", 1, -600.0)]
    for which in ("extrinsic", "linearize"):
        assert raw_call(CB, case, which)[0] == L.OK
        for m in mods:
            rc, untouched = raw_call(CB, case, which, **m)
            assert rc == L.ERR_ARG and untouched, (which, list(m))
        for kw in (dict(max_iterations=0), dict(max_error_px=-1.0), dict(min_eig_ratio=-1e-9), dict(eps_rot=-1.0), dict(eps_trans=-1.0),
                   dict(min_records=-1), dict(loss_scale_px=-2.0), dict(loss_kind=9), dict(eps_rot=np.nan)):
            rc, untouched = raw_call(CB, case, which, o=CB.calib_opts(**kw))
            assert rc == L.ERR_ARG and untouched, (which, kw)
    with pytest.raises(TypeError):
        CB.calib_opts(hypotheses=3)
    with pytest.raises(L.LvbaError) as e:
        CB.refine_jobs(records_of(case), (case["img_a"], case["img_b"]), case["poses"], case["intr"], case["R0"], case["t0"], max_iterations=0)
    assert e.value.code == L.ERR_ARG
    assert raw_call(CB, case, "extrinsic")[0] == L.OK                             # and the library is usable afterwards


def _with(a, i, v):
    a = a.copy()
    a.reshape(-1)[i] = v
    return a


def test_a_second_round_ends_nearer_the_planted_extrinsic(CB, pkg):
    """pipeline.calibrate_extrinsic on the small room sequence with rendered depth images, from an extrinsic 2 degrees and 10.8 cm
    off: the first round's depths were read through the wrong extrinsic, so rounds = 2 ends nearer the true one than rounds = 1."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    V = importlib.import_module("global-lvba_amd.visual")
    voxel = importlib.import_module("global-lvba_amd.voxel")
    d = cc.room_sequence()
    R0, t0 = co.perturb(cc.ROOM_RCI.reshape(9), cc.ROOM_TCI, cc.ROOM_PLANT)
    c = pipe.DEFAULTS
    err = {}
    with voxel.Scans(d["clouds"]) as scans:
        render = lambda Rk, tk: V.DepthImages.render(scans, d["poses"], d["times"], d["times"], Rk, tk, cc.ROOM_INTR, cc.ROOM_W, cc.ROOM_H,
                                                     half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
        for rounds in (1, 2):
            rep = pipe.calibrate_extrinsic(d["kps"], d["pairs"], d["matches"], d["poses"], R0.reshape(3, 3), t0, cc.ROOM_INTR, render=render,
                                           rounds=rounds)
            e = co.left_difference(np.array(rep["Rci"]), np.array(rep["tci"]), cc.ROOM_RCI, cc.ROOM_TCI)
            err[rounds] = (np.linalg.norm(e[:3]), np.linalg.norm(e[3:]), np.linalg.norm(e))
            print("rounds", rounds, rep["status"], "n_held", rep["n_held"], "records", rep["n_records"], "rmse %.3f px" % rep["rmse_px"],
                  "error %.5f deg %.5f m" % (np.degrees(err[rounds][0]), err[rounds][1]), "std", rep["std_rot_deg"], rep["std_trans_m"],
                  "iterations", [r["iterations"] for r in rep["rounds"]])
            assert rep["status"] == "converged" and rep["n_held"] == 0 and len(rep["rounds"]) == rounds and rep["n_records"] > 1500
            assert abs(rep["rounds"][0]["rotation_deg"] - 2.0) < 0.5             # the first round takes most of the planted turn back
    assert err[1][2] < 0.2 * np.linalg.norm(cc.ROOM_PLANT)
    assert err[2][0] < err[1][0] and err[2][1] < err[1][1]                       # nearer in rotation and in translation


def test_run_full_pipeline_reports_without_touching_the_rest(CB, pkg):
    """run_full_pipeline(calibrate_extrinsic=True) on the small loop sequence reports what the direct call reports and leaves every
    other output byte-equal to the run without the keyword."""
    import test_gpu_mapq as tm
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    V = importlib.import_module("global-lvba_amd.visual")
    voxel = importlib.import_module("global-lvba_amd.voxel")
    d = tm._dataset()
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    c = dict(pipe.DEFAULTS, **cfg)
    odo = d["odo"]
    args = (d["clouds"], odo, d["times"], d["img_t"], odo, tm.RCB, tm.TCI, tm.INTR, tm.W, tm.H, d["kps"], d["pairs"], d["matches"])
    on = pipe.run_full_pipeline(*args, enable_lidar_ba=False, calibrate_extrinsic=dict(max_iterations=5), **cfg)
    plain = pipe.run_full_pipeline(*args, enable_lidar_ba=False, **cfg)
    cam = pipe.update_camera_poses_from_lidar(odo, odo, d["times"], d["img_t"], odo)
    with voxel.Scans(d["clouds"]) as scans:
        render = lambda Rk, tk: V.DepthImages.render(scans, odo, d["times"], d["img_t"], Rk, tk, tm.INTR, tm.W, tm.H,
                                                     half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
        direct = pipe.calibrate_extrinsic(d["kps"], d["pairs"], d["matches"], cam, tm.RCB, tm.TCI, tm.INTR, render=render, max_iterations=5)
    print("loop sequence:", direct["status"], "records", direct["n_records"], "moved %.4f deg %.4f m" % (direct["rotation_deg"], direct["translation_m"]))
    assert "extrinsic" not in plain and on["extrinsic"].pop("applied") is False
    assert on["extrinsic"] == direct and direct["n_records"] > 1000
    assert on["poses"].tobytes() == plain["poses"].tobytes() and set(on) == set(plain) | {"extrinsic"}
    for k in ("Rcw", "tcw", "landmarks", "landmark_valid", "track_status", "Rcw_lidar", "tcw_lidar", "Rcw_before", "tcw_before"):
        assert np.asarray(on["visual"][k]).tobytes() == np.asarray(plain["visual"][k]).tobytes(), k
