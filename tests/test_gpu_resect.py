"""GPU tests of the camera resectioning (lvba_resect_*, the resect module, pipeline.check_cameras / localize_images) against the
numpy restatement (tests/resect_oracle.py) on the shared fixtures (tests/resect_cases.py).  A hypothesis is formed
from +, -, *, / and sqrt in one order and the file is built without contraction: poses, counts, winners and inlier lists are
compared exactly.  Only the refinement, whose sums are a tree on the device, is held to the tolerance measured in
test_resect_host.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import resect_cases as rc
import resect_oracle as ro
from test_resect_host import ORDER_TOL_R, ORDER_TOL_T, REFIT_TOL_R, REFIT_TOL_T, emul, host_job  # noqa: F401 (emul is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def RS(pkg):
    return importlib.import_module("global-lvba_amd.resect")


def intr_of(case):
    return case["scene"]["intr"]


def run_batch(RS, cases, **over):
    o = dict(cases[0]["opts"], **over)
    return RS.resect_images([c["uv"] for c in cases], [c["world"] for c in cases], intr_of(cases[0]), ids=[c["id"] for c in cases], **o)


def check_batch_exact(got, cases, **over):
    (ginl, rep), rs = got, [rc.oracle_job(c, **over) for c in cases]
    np.testing.assert_array_equal(rep["status"], [r["status"] for r in rs])
    np.testing.assert_array_equal(rep["best_h"], [r["best_h"] for r in rs])
    np.testing.assert_array_equal(rep["n_inliers"], [r["n_inliers"] for r in rs])
    np.testing.assert_array_equal(rep["Rcw"].reshape(-1, 9), np.array([r["R"] for r in rs]).reshape(-1, 9))
    np.testing.assert_array_equal(rep["tcw"], np.array([r["t"] for r in rs]).reshape(-1, 3))
    for g, r, c in zip(ginl, rs, cases):
        np.testing.assert_array_equal(g, np.flatnonzero(r["mask"]), err_msg=c["name"])


def test_hypotheses_equal_the_oracle(RS):
    """every hypothesis's R, t and count of every fixture, bit for bit: the correspondence-count ladder (either side of the sample
    size, of min_inliers, of the wavefront and of the LDS chunk), H either side of the hypothesis block, unusable
    correspondences, one correspondence repeated, two ids, the plane"""
    n_bad = 0
    for case in rc.all_gpu_cases():
        R, t, count, _, _ = rc.oracle_hypotheses(case)
        gR, gt, gcount = RS.hypotheses(case["id"], case["uv"], case["world"], intr_of(case), **case["opts"])
        np.testing.assert_array_equal(gR.reshape(-1, 9), R, err_msg=case["name"])
        np.testing.assert_array_equal(gt, t, err_msg=case["name"])
        np.testing.assert_array_equal(gcount, count, err_msg=case["name"])
        n_bad += int((count == -1).sum())
    assert n_bad > 0


def test_images_without_refinement_equal_the_oracle(RS):
    g, p = rc.general(), rc.planar()
    for cases in (g["sizes"], g["mixed"], g["special"] + g["two_ids"], g["claims"], p["claims"]):
        got = run_batch(RS, cases, refine_rounds=0)
        check_batch_exact(got, cases, refine_rounds=0)
    # the batch against single jobs, reversed, and called twice
    cases = g["mixed"]
    (inl, rep) = run_batch(RS, cases, refine_rounds=0)
    (inl2, rep2) = run_batch(RS, cases, refine_rounds=0)
    (rinl, rrep) = run_batch(RS, cases[::-1], refine_rounds=0)
    for k in ("Rcw", "tcw", "status", "n_inliers", "best_h", "rmse_px", "information"):
        assert rep[k].tobytes() == rep2[k].tobytes(), k
        assert rep[k].tobytes() == rrep[k][::-1].tobytes(), k
    for a, b, c in zip(inl, inl2, rinl[::-1]):
        np.testing.assert_array_equal(a, b); np.testing.assert_array_equal(a, c)
    for j in (0, 4, 12, 17, 39):
        (sinl, srep) = run_batch(RS, cases[j:j + 1], refine_rounds=0)
        np.testing.assert_array_equal(sinl[0], inl[j])
        for k in ("Rcw", "tcw", "status", "n_inliers", "best_h", "rmse_px", "information"):
            assert srep[k][0].tobytes() == rep[k][j].tobytes(), (j, k)


def test_images_with_refinement(RS, emul):
    g, p = rc.general(), rc.planar()
    worst_o = [0.0, 0.0]
    for cases in (g["claims"], p["claims"], g["mixed"], g["sizes"]):
        inl, rep = run_batch(RS, cases)
        inl0, rep0 = run_batch(RS, cases, refine_rounds=0)
        for j, case in enumerate(cases):
            r = rc.oracle_job(case)
            assert rep["status"][j] == r["status"] and rep["best_h"][j] == r["best_h"], case["name"]
            assert rep["n_inliers"][j] >= rep0["n_inliers"][j], case["name"]          # a refit is kept only if it loses nothing
            if r["best_h"] < 0:
                continue
            # every refined pose, those over a handful of inliers included, against the host build of the same header: only the
            # order of the sums differs
            h = host_job(emul, case)
            assert rep["n_inliers"][j] == h["n_inliers"], case["name"]
            oR, ot = ro.pose_difference(rep["Rcw"][j], rep["tcw"][j], h["R"], h["t"])
            worst_o[0], worst_o[1] = max(worst_o[0], oR), max(worst_o[1], ot)
            assert oR <= ORDER_TOL_R and ot <= ORDER_TOL_T, (case["name"], oR, ot)
            # the mask is the oracle's score of the returned pose
            mask = ro.score(rep["Rcw"][j].reshape(9), rep["tcw"][j], case["rec"], intr_of(case), 8.0)
            assert mask.sum() == rep["n_inliers"][j]
            np.testing.assert_array_equal(inl[j], np.flatnonzero(mask) if rep["status"][j] == ro.OK else [], err_msg=case["name"])
            if r["count0"] >= 30:
                dR, dt = ro.pose_difference(rep["Rcw"][j], rep["tcw"][j], r["R"], r["t"])
                print(case["name"], "refit against the oracle's: |dR|_F %.3g  |dt|/|t| %.3g" % (dR, dt))
                assert dR <= REFIT_TOL_R and dt <= REFIT_TOL_T, case["name"]
                assert rep["n_inliers"][j] == r["n_inliers"]
                assert abs(rep["rmse_px"][j] - r["rmse_px"]) < 1e-9
                np.testing.assert_allclose(rep["information"][j], r["information"], rtol=0, atol=1e-9 * np.abs(r["information"]).max())
    print("largest difference from the host emulation's refinement: |dR|_F %.3g  |dt|/|t| %.3g" % tuple(worst_o))
    # the planted claims: 40 % outliers in general position, 60 % on the single plane, exactly the planted set
    for cases in (g["claims"], p["claims"]):
        inl, rep = run_batch(RS, cases)
        for j, case in enumerate(cases):
            assert rep["status"][j] == RS.OK
            np.testing.assert_array_equal(inl[j], np.flatnonzero(case["planted"]), err_msg=case["name"])


def test_score_equals_the_oracle(RS):
    for case in rc.general()["claims"] + rc.planar()["claims"]:
        Rt, tt = rc.truth(case)
        r = rc.oracle_job(case)
        for R, t, rho in ((Rt, tt, 8.0), (r["R0"], r["t0"], 8.0), (r["R0"], r["t0"], 1.0)):
            np.testing.assert_array_equal(RS.score(case["uv"], case["world"], intr_of(case), R, t, max_error_px=rho),
                                          ro.score(R, t, case["rec"], intr_of(case), rho))
        assert RS.score(case["uv"], case["world"], intr_of(case), Rt, tt)[case["planted"]].all()
    assert len(RS.score(np.zeros((0, 2)), np.zeros((0, 3)), intr_of(case), Rt, tt)) == 0


def _analytic_depth(sc):
    """per-pixel depth of the corner scene's two planes in every view, by undistorting each pixel and intersecting its ray"""
    W, H = sc["width"], sc["height"]
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    intr = sc["intr"]
    fx, fy, cx, cy, k1, k2, p1, p2 = intr
    xd, yd = (uu.astype(np.float64) - cx) / fx, (vv.astype(np.float64) - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(8):                                   # trk_undistort's iteration, vectorised (depth is fp32: rounding is of no account)
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * r2 * r2
        x, y = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / radial, (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / radial
    out = np.zeros((4, H, W), np.float32)
    planes = ((np.array([-0.8, 0.0, 1.0]), 9.0, -1.0), (np.array([0.6, 0.0, 1.0]), 9.0, 1.0))   # n . X = d, valid where sign * X_x > 0
    for v in range(4):
        R, t = sc["Rcw"][v], sc["tcw"][v]
        ray = np.stack([x, y, np.ones_like(x)], -1) @ R                  # R^T (x, y, 1): the ray in the world
        centre = -R.T @ t
        best = np.full((H, W), np.inf)
        for n, d, sign in planes:
            lam = (d - n @ centre) / (ray @ n)
            Xw = centre + lam[..., None] * ray
            ok = (lam > 0) & (sign * Xw[..., 0] > 0)
            best = np.where(ok & (lam < best), lam, best)
        out[v] = np.where(np.isfinite(best), best, 0.0)
    return out


def test_lift_equals_the_matchers_points(RS, pkg):
    V = importlib.import_module("global-lvba_amd.visual")
    M = importlib.import_module("global-lvba_amd.match")
    sc = rc.corner()
    depth = V.DepthImages.upload(_analytic_depth(sc))
    try:
        pts = RS.lift_keypoints(depth, sc["keypoints"], sc["intr"], sc["Rcw"], sc["tcw"])
        with M.Matcher(sc["descriptors"]) as m:
            m.set_geometry(sc["keypoints"], sc["intr"], sc["Rcw"], sc["tcw"])
            m.set_depth(depth)
            want = m.points()
        got = np.concatenate(pts)
        assert got.tobytes() == want.tobytes()
        has = ~np.isnan(got[:, 0])
        assert has.mean() > 0.95
        assert np.abs(got[has] - np.concatenate([sc["points"]] * 4)[has]).max() < 0.05       # 0.3 px of noise at nine metres
        with pytest.raises(pkg._lib.LvbaError) as e:                      # a depth set of another image count
            RS.lift_keypoints(depth, sc["keypoints"][:3], sc["intr"], sc["Rcw"][:3], sc["tcw"][:3])
        assert e.value.code == pkg._lib.ERR_ARG
    finally:
        depth.close()


def test_error_paths_and_capacity(RS, pkg):
    L = pkg._lib
    g = rc.general()
    case = g["claims"][0]
    uv, world, intr = case["uv"], case["world"], intr_of(case)
    bad_intr = intr.copy(); bad_intr[0] = 0.0
    nan_intr = intr.copy(); nan_intr[4] = np.nan
    for kw in (dict(ids=[-1]), dict(hypotheses=0), dict(refine_rounds=-1), dict(min_inliers=-1), dict(max_error_px=0.0),
               dict(max_error_px=np.inf)):
        with pytest.raises(L.LvbaError) as e:
            RS.resect_images([uv], [world], intr, **kw)
        assert e.value.code == L.ERR_ARG, kw
    for bad in (bad_intr, nan_intr):
        with pytest.raises(L.LvbaError) as e:
            RS.resect_images([uv], [world], bad)
        assert e.value.code == L.ERR_ARG
    with pytest.raises(L.LvbaError) as e:                                  # a repeated id
        RS.resect_images([uv, uv], [world, world], intr, ids=[3, 3])
    assert e.value.code == L.ERR_ARG and "twice" in str(e.value)
    # a refusal writes nothing: the C call with every output filled beforehand
    lib = L.load()
    ids, off = np.array([3, 3], np.int32), np.array([0, len(uv), 2 * len(uv)], np.int64)
    uv2, w2 = np.ascontiguousarray(np.vstack([uv, uv])), np.ascontiguousarray(np.vstack([world, world]))
    outs = [np.full(3, -7, np.int64), np.full(2 * len(uv), -7, np.int32), np.full(18, -7.0), np.full(6, -7.0), np.full(2, -7, np.int32),
            np.full(2, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7.0), np.full(72, -7.0)]
    o = RS.resect_opts()
    rcode = lib.lvba_resect_images(0, 2, ids.ctypes.data, off.ctypes.data, uv2.ctypes.data, w2.ctypes.data, intr.ctypes.data, C.byref(o),
                                   2 * len(uv), *[a.ctypes.data for a in outs])
    assert rcode == L.ERR_ARG and all((a == -7).all() for a in outs)
    with pytest.raises(L.LvbaError):
        RS.hypotheses(-2, uv, world, intr)
    with pytest.raises(L.LvbaError):
        RS.score(uv, world, intr, np.eye(3), np.zeros(3), max_error_px=-1.0)
    with pytest.raises(TypeError):
        RS.resect_images([uv], [world], intr, method=1)
    # a capacity that is too small: the true offsets, the first `capacity` inliers
    cases = g["mixed"][12:18]
    flat_uv = np.concatenate([c["uv"] for c in cases]); flat_w = np.concatenate([c["world"] for c in cases])
    off = np.cumsum([0] + [len(c["uv"]) for c in cases])
    ids = [c["id"] for c in cases]
    full, foff, _ = RS.resect_images_csr(ids, off, flat_uv, flat_w, intr, hypotheses=rc.H_SMALL)
    part, poff, _ = RS.resect_images_csr(ids, off, flat_uv, flat_w, intr, capacity=37, hypotheses=rc.H_SMALL)
    assert foff[-1] == len(full) > 37 and len(part) == 37
    np.testing.assert_array_equal(poff, foff); np.testing.assert_array_equal(part, full[:37])
    none, noff, _ = RS.resect_images_csr(ids, off, flat_uv, flat_w, intr, capacity=0, hypotheses=rc.H_SMALL)
    assert len(none) == 0 and noff[-1] == foff[-1]
    o = RS.resect_opts()
    assert (o.hypotheses, o.refine_rounds, o.min_inliers, o.max_error_px, o.seed) == (1024, 2, 30, 8.0, 0)
    assert C.sizeof(L.ResectOpts) == 32
    inl, rep = RS.resect_images([], [], intr)                               # no job at all
    assert inl == [] and len(rep["status"]) == 0
    other = RS.resect_images([uv], [world], intr, seed=1)[1]                # another stream, a valid result
    assert other["status"][0] == RS.OK


def test_localize_images_on_the_corner_scene(RS, pkg):
    """View 3 is held out: its keypoints are matched unguided against the three map views, whose keypoints carry the points lifted
    through analytic depth images; it comes back OK with the planted inliers and as near the truth as the oracle on the same
    correspondences."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    V = importlib.import_module("global-lvba_amd.visual")
    sc = rc.corner()
    depth = V.DepthImages.upload(_analytic_depth(sc)[:3])
    try:
        map_points = RS.lift_keypoints(depth, sc["keypoints"][:3], sc["intr"], sc["Rcw"][:3], sc["tcw"][:3])
    finally:
        depth.close()
    Rq, tq, report = pipe.localize_images(sc["keypoints"][3:], sc["descriptors"][3:], sc["keypoints"][:3], sc["descriptors"][:3],
                                          map_points, sc["intr"])
    assert report["images"][0]["status"] == "ok" and report["n_images_ok"] == 1
    corr = report["correspondences"][0]
    planted = corr["keypoint"] == corr["map_keypoint"]                      # keypoint k of every view is point k
    assert len(planted) > 1000 and planted.mean() > 0.9
    np.testing.assert_array_equal(corr["inlier"], planted)
    uv = sc["keypoints"][3][corr["keypoint"]]
    world = np.concatenate([map_points[c][corr["map_keypoint"][corr["map_image"] == c]] for c in range(3)])
    want = ro.resect(ro.records(sc["intr"], uv, world), 0, sc["intr"])
    dR, dt = ro.pose_difference(Rq[0], tq[0], want["R"], want["t"])
    print("localisation against the oracle's: |dR|_F %.3g  |dt|/|t| %.3g;  from the truth: %s (oracle %s)" % (
        dR, dt, ro.pose_offset(Rq[0], tq[0], sc["Rcw"][3], sc["tcw"][3]), ro.pose_offset(want["R"], want["t"], sc["Rcw"][3], sc["tcw"][3])))
    assert want["status"] == ro.OK and dR <= REFIT_TOL_R and dt <= REFIT_TOL_T
    a, d = ro.pose_offset(Rq[0], tq[0], sc["Rcw"][3], sc["tcw"][3])
    assert a < 0.05 and d < 0.01


DISPLACED, SHIFT_M, TURN_DEG = 5, 0.06, 0.4


def test_pipeline_checks_the_cameras(RS, pkg):
    """run_full_pipeline(check_cameras=True) on the small sequence at its true poses, the pose input of image DISPLACED moved by
    SHIFT_M and turned by TURN_DEG: that image's reported offset is the displacement to within the oracle's own error on the same
    correspondences, and the other images report offsets no larger than the oracle's."""
    import test_gpu_mapq as tm
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    synth = importlib.import_module("global-lvba_amd.synth")
    V = importlib.import_module("global-lvba_amd.visual")
    voxel = importlib.import_module("global-lvba_amd.voxel")
    d = tm._dataset()
    s = synth.make_scans(12, 40000, room=(14, 10, 4), n_panels=0, n_blobs=0, clutter_frac=0.0, seed=62, rot_sigma_deg=0.15, trans_sigma=0.04)
    gt = np.asarray(s["poses_gt"], np.float64).reshape(-1, 12)
    img_poses = gt.copy()
    w = np.radians(TURN_DEG) * np.array([0.0, 0.6, 0.8])
    img_poses[DISPLACED, :9] = (ro.rodrigues(w) @ gt[DISPLACED, :9].reshape(3, 3)).reshape(9)
    img_poses[DISPLACED, 9:] += SHIFT_M * np.array([0.6, -0.8, 0.0])
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    args = (d["clouds"], gt, d["times"], d["img_t"], img_poses, tm.RCB, tm.TCI, tm.INTR, tm.W, tm.H, d["kps"], d["pairs"], d["matches"])
    out = pipe.run_full_pipeline(*args, enable_lidar_ba=False, enable_visual_ba=False, check_cameras=True, **cfg)
    chk = out["camera_check"]
    assert chk["n_images"] == 12 and "visual" not in out
    # the same correspondences on the host, for the oracle
    cam = pipe.update_camera_poses_from_lidar(gt, gt, d["times"], d["img_t"], img_poses)
    Rk, tk = pipe.camera_from_imu(cam, tm.RCB, tm.TCI)
    Rt, tt = pipe.camera_from_imu(pipe.update_camera_poses_from_lidar(gt, gt, d["times"], d["img_t"], gt), tm.RCB, tm.TCI)
    c = dict(pipe.DEFAULTS, **cfg)
    with voxel.Scans(d["clouds"]) as scans:
        depth = V.DepthImages.render(scans, gt, d["times"], d["img_t"], Rk, tk, tm.INTR, tm.W, tm.H, half_window_s=c["depth_half_window_s"],
                                     voxel_size=c["depth_voxel"])
        try:
            points = RS.lift_keypoints(depth, d["kps"], tm.INTR, Rk, tk)
        finally:
            depth.close()
    kp, world = pipe.correspondences_from_matches(d["pairs"], d["matches"], points)
    n_ok = 0
    for j, e in enumerate(chk["images"]):
        want = ro.resect(ro.records(tm.INTR, d["kps"][j][kp[j]], world[j]), j, tm.INTR)
        assert e["status"] == RS.STATUS_NAMES[want["status"]] and e["n_inliers"] == want["n_inliers"], j
        if want["status"] != ro.OK:
            continue
        n_ok += 1
        oa, od = ro.pose_offset(want["R"], want["t"], Rt[j], tt[j])         # the oracle's own error on this job
        ga, gd = ro.pose_offset(Rk[j], tk[j], Rt[j], tt[j])                 # how far the given pose is from the truth
        print("image", j, "reported %.4f deg %.4f m; given pose off by %.4f deg %.4f m; oracle's error %.4f deg %.4f m" % (
            e["rotation_deg"], e["translation"], ga, gd, oa, od))
        slack_a, slack_d = 1e-9, 1e-9                                       # the refit's tolerance, in these units
        assert abs(e["rotation_deg"] - ga) <= oa + slack_a and abs(e["translation"] - gd) <= od + slack_d, j
    assert n_ok >= 10 and chk["images"][DISPLACED]["status"] == "ok"
    assert chk["n_images_ok"] == n_ok and chk["median_translation"] == np.median([e["translation"] for e in chk["images"] if e["status"] == "ok"])
