"""GPU tests of the map-quality metrics (lvba_mapq_scans / lvba_mapq_points, global-lvba_amd/mapq.py): every query of a small
scan set against the brute-force restatement (tests/mapq_oracle.py), the lattice whose neighbours lie exactly one radius away
on cell faces, run-to-run identity, the argument checks and the pipeline hook."""
import ctypes as C
import importlib

import numpy as np
import pytest

import mapq_oracle as mo

pytestmark = pytest.mark.gpu

SUMMARY = ("n_points", "n_queries", "n_valid", "mme", "mpv", "mean_neighbors")


@pytest.fixture(scope="module")
def mq(pkg):
    return importlib.import_module("global-lvba_amd.mapq")


@pytest.fixture(scope="module")
def case(pkg):
    c = mo.scan_case()
    with pkg.Scans(c["clouds"]) as scans:
        yield dict(c, scans=scans)


def same_bytes(a, b):
    for k in SUMMARY + ("entropy", "plane_var", "normal", "count"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


@pytest.mark.parametrize("name", ["gt", "noisy"])
@pytest.mark.parametrize("stride", [1, 3])
def test_every_query_matches_the_oracle(mq, case, name, stride):
    ref = mo.strided(case["ref"][name], stride)
    got = mq.map_quality_scans(case["scans"], case["poses"][name], radius=0.3, min_neighbors=8, query_stride=stride, per_point=True)
    fig = mo.check_parity(got, ref, 0.3)
    print(name, stride, fig, {k: got[k] for k in SUMMARY})
    assert fig["max_bound"] <= 1.1e-10 and fig["sharp_share"] >= 0.7, fig
    assert (got["n_points"], got["n_queries"], got["n_valid"]) == (6000, ref["n_queries"], ref["n_valid"])
    for k in ("mme", "mpv", "mean_neighbors"):
        assert abs(got[k] - ref[k]) <= 1e-10 * abs(ref[k]), (k, got[k], ref[k])


def test_lattice_one_radius_apart_on_cell_faces(mq):
    base = None
    for shift in ((0, 0, 0), (1000.25, -517.5, 0)):
        p = mo.lattice(shift)
        ref = mo.metrics(p, 0.25, 4)
        got = mq.map_quality_points(p, radius=0.25, min_neighbors=4, per_point=True)
        assert [int((got["count"] == c).sum()) for c in (4, 5, 6, 7)] == [8, 48, 96, 64]
        assert np.array_equal(got["count"], ref["count"]) and np.array_equal(np.isfinite(got["entropy"]), ref["valid"])
        inner = got["count"] == 7
        assert np.abs(got["entropy"][inner] - mo.LATTICE_INTERIOR_ENTROPY).max() <= 1e-12
        base = got["count"] if base is None else base
        assert np.array_equal(got["count"], base)


def test_same_bytes_twice_and_from_the_downloaded_cloud(mq, case):
    kw = dict(radius=0.3, min_neighbors=8, per_point=True)
    a = mq.map_quality_scans(case["scans"], case["poses"]["noisy"], **kw)
    b = mq.map_quality_scans(case["scans"], case["poses"]["noisy"], **kw)
    assert same_bytes(a, b)
    c = mq.map_quality_points(case["world"]["noisy"], **kw)       # the world cloud as the coloured map forms and downloads it
    assert same_bytes(a, c)
    # a query's sums do not depend on which other points are queries
    s = mq.map_quality_scans(case["scans"], case["poses"]["noisy"], query_stride=3, **kw)
    assert s["entropy"].tobytes() == a["entropy"][::3].tobytes() and s["normal"].tobytes() == a["normal"][::3].tobytes()


def test_nan_point_and_frame_sub_range(pkg, mq, case):
    clouds = [c.copy() for c in case["clouds"]]
    clouds[1][700] = (np.nan, 0.0, 0.0)
    clouds[2][3] = (0.0, np.inf, 0.0)
    world = mo.world_points(clouds, case["poses"]["gt"])
    bad = [1500 + 700, 3000 + 3]
    assert not np.isfinite(world[bad]).all(1).any()
    ref = mo.metrics(world, 0.3, 8)
    with pkg.Scans(clouds) as sc:
        got = mq.map_quality_scans(sc, case["poses"]["gt"], per_point=True)
        mo.check_parity(got, ref, 0.3)
        assert list(got["count"][bad]) == [0, 0] and not np.isfinite(got["entropy"][bad]).any()
        assert (got["count"] <= case["ref"]["gt"]["count"]).all() and (got["count"] < case["ref"]["gt"]["count"]).any()
        assert abs(got["mean_neighbors"] - ref["mean_neighbors"]) <= 1e-10 * ref["mean_neighbors"]
        sub = mq.map_quality_scans(sc, case["poses"]["gt"][1:3], frame_begin=1, n_frames=2, query_stride=2, per_point=True)
    ref2 = mo.metrics(world[1500:4500], 0.3, 8, 2)
    mo.check_parity(sub, ref2, 0.3)
    assert (sub["n_points"], sub["n_queries"], sub["n_valid"]) == (3000, 1500, ref2["n_valid"])
    assert abs(sub["mme"] - ref2["mme"]) <= 1e-10 * abs(ref2["mme"])


def test_argument_errors_leave_the_library_usable(pkg, mq, case):
    L = pkg._lib
    lib = L.load()
    sc, x = case["scans"], case["poses"]["gt"]
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(min_neighbors=3),
               dict(query_stride=0), dict(frame_begin=-1, n_frames=1), dict(frame_begin=3, n_frames=2), dict(frame_begin=0, n_frames=0)):
        poses = x[:kw["n_frames"]] if "n_frames" in kw else x
        with pytest.raises(L.LvbaError) as e:
            mq.map_quality_scans(sc, poses, **kw)
        assert e.value.code == L.ERR_ARG, kw
    bad = x.copy(); bad[2, 10] = np.nan
    with pytest.raises(L.LvbaError) as e:
        mq.map_quality_scans(sc, bad)
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.LvbaError) as e:
        mq.map_quality_points(np.zeros((5, 3), np.float32), radius=-2.0)
    assert e.value.code == L.ERR_ARG
    o, s = L.MapqOpts(), L.MapqSummary()
    lib.lvba_mapq_default_opts(C.byref(o))
    assert (o.radius, o.min_neighbors, o.query_stride) == (0.3, 8, 1)
    xyz = np.zeros((4, 3), np.float32)
    assert lib.lvba_mapq_points(0, 4, xyz.ctypes.data, C.byref(o), None, None, None, None, None) == L.ERR_ARG      # no summary
    assert lib.lvba_mapq_points(0, 4, None, C.byref(o), C.byref(s), None, None, None, None) == L.ERR_ARG            # no points
    assert lib.lvba_mapq_points(0, -1, xyz.ctypes.data, C.byref(o), C.byref(s), None, None, None, None) == L.ERR_ARG
    assert lib.lvba_mapq_scans(None, x.reshape(-1), 0, 4, C.byref(o), C.byref(s), None, None, None, None) == L.ERR_ARG
    assert lib.lvba_mapq_scans(sc._h, x.reshape(-1), 0, 4, C.byref(o), None, None, None, None, None) == L.ERR_ARG
    assert lib.lvba_mapq_points(0, 4, xyz.ctypes.data, None, C.byref(s), None, None, None, None) == L.OK            # default options
    # a point beyond 2^20 cells is refused, and the call after it works
    far = np.array([[0, 0, 0], [0.3 * 2.0 ** 20, 0, 0]], np.float32)
    with pytest.raises(L.LvbaError) as e:
        mq.map_quality_points(far)
    assert e.value.code == L.ERR_ARG
    ok = mq.map_quality_points(far, radius=0.6)
    assert ok["n_points"] == 2 and ok["n_valid"] == 0 and np.isnan(ok["mme"]) and ok["mean_neighbors"] == 1.0
    again = mq.map_quality_scans(sc, x)
    assert again["n_valid"] == case["ref"]["gt"]["n_valid"]
    assert mq.map_quality_points(np.zeros((0, 3), np.float32))["n_queries"] == 0


# ------------------------------------------------------------------------------------------------------------------ pipeline
RCB = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
TCI = np.array([0.02, 0.05, -0.03])
INTR = np.array([300.0, 298.0, 240.0, 180.0, -0.076160, 0.123001, -0.00113, 0.000251])
W, H = 480, 360


def _dataset(n_frames=12, pts=40000, n_land=400, seed=62):
    """The small sequence of tests/test_gpu_pipeline.py (its generator, at the size of its dataset-directory test)."""
    from oracle import track_oracle as to
    synth = importlib.import_module("global-lvba_amd.synth")
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    s = synth.make_scans(n_frames, pts, room=(14, 10, 4), n_panels=0, n_blobs=0, clutter_frac=0.0, seed=seed, rot_sigma_deg=0.15,
                         trans_sigma=0.04)
    gt = np.asarray(s["poses_gt"], np.float64).reshape(-1, 12)
    odo = np.asarray(s["poses"], np.float64).reshape(-1, 12)
    times = 50.0 + 0.1 * np.arange(n_frames)
    img_t = times + 0.004
    rng = np.random.default_rng(seed)
    world = np.concatenate([c[:, :3].astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:] for c, T in zip(s["clouds"], gt)])
    X = world[rng.choice(len(world), n_land, replace=False)]
    Rcw_gt, tcw_gt = pipe.camera_from_imu(gt, RCB, TCI)
    kps, lm_of = [], []
    for m in range(n_frames):
        k, ids = [], []
        for li, x in enumerate(X):
            p = to.project(INTR, Rcw_gt[m], tcw_gt[m], x)
            if p is not None and 3 < p[0] < W - 4 and 3 < p[1] < H - 4 and (Rcw_gt[m] @ x + tcw_gt[m])[2] < 12.0:
                k.append(np.float32(p) + np.float32(0.4 * rng.standard_normal(2))); ids.append(li)
        kps.append(np.array(k, np.float32).reshape(-1, 2)); lm_of.append(ids)
    pairs, matches = [], []
    for i in range(n_frames):
        for j in range(i + 1, min(n_frames, i + 7)):
            pos_j = {li: kj for kj, li in enumerate(lm_of[j])}
            m = [(ki, pos_j[li]) for ki, li in enumerate(lm_of[i]) if li in pos_j]
            if m:
                pairs.append((i, j)); matches.append(np.array(m, np.int64))
    return dict(clouds=s["clouds"], odo=odo, times=times, img_t=img_t, kps=kps, pairs=pairs, matches=matches)


def test_pipeline_reports_map_quality(pkg, mq):
    """run_full_pipeline(map_quality=...) returns the summaries of direct calls at the refined and at the original poses, and
    changes nothing else; both agree with the oracle on the same (strided) queries.  On this sequence (480 000 points, 100
    queries) the oracle has MME -3.676 after against -2.869 before (MPV 4.35e-4 against 1.57e-3): the refined map is the
    sharper one, and that is asserted."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = _dataset()
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], RCB, TCI, INTR, W, H, d["kps"], d["pairs"], d["matches"])
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    kw = dict(radius=0.3, min_neighbors=8, query_stride=4801)
    on = pipe.run_full_pipeline(*args, map_quality=kw, **cfg)
    off = pipe.run_full_pipeline(*args, map_quality=False, **cfg)
    plain = pipe.run_full_pipeline(*args, **cfg)
    assert "map_quality" not in off and "map_quality" not in plain
    for a, b in ((off, plain), (on, plain)):
        assert a["poses"].tobytes() == b["poses"].tobytes()
        for k in ("Rcw", "tcw", "landmarks", "landmark_valid", "track_status"):
            assert np.asarray(a["visual"][k]).tobytes() == np.asarray(b["visual"][k]).tobytes(), k
    clouds = [np.ascontiguousarray(np.asarray(c, np.float32)[:, :3]) for c in d["clouds"]]
    q = on["map_quality"]
    with pkg.Scans(clouds) as sc:
        direct = pipe.map_quality(sc, on["poses"], d["odo"], **kw)
    ref = {}
    for name, x in (("after", on["poses"]), ("before", d["odo"])):
        assert {k: q[name][k] for k in SUMMARY} == {k: direct[name][k] for k in SUMMARY}
        ref[name] = r = mo.metrics(mo.world_points(clouds, x), **kw)
        assert (q[name]["n_points"], q[name]["n_queries"], q[name]["n_valid"]) == (480000, 100, r["n_valid"])
        for k in ("mme", "mpv", "mean_neighbors"):
            assert abs(q[name][k] - r[k]) <= 1e-10 * abs(r[k]), (name, k, q[name][k], r[k])
    print("mme after / before", q["after"]["mme"], q["before"]["mme"], "mpv", q["after"]["mpv"], q["before"]["mpv"])
    assert ref["after"]["mme"] < ref["before"]["mme"] - 0.5 and ref["after"]["mpv"] < ref["before"]["mpv"]
    assert q["after"]["mme"] < q["before"]["mme"] and q["after"]["mpv"] < q["before"]["mpv"]
