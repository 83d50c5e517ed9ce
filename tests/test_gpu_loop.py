"""GPU tests of the loop-closure detection: submap sets (lvba_submaps_*), registration against a submap per job
(lvba_register_*_submaps), the candidate search (lvba_loop_candidates) and pipeline.find_loop_closures, against each submap's own
map, the numpy restatements (tests/register_oracle.py, tests/loop_oracle.py) and the shared fixture (tests/loop_cases.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import loop_cases as lc
import loop_oracle as lo
import register_oracle as ro
from test_loop_host import search_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg):
    s = lc.scans()
    sc = pkg.Scans(s["clouds"])
    P = lc.truth()
    sm = sc.submaps(P, lc.S, lc.VS, lc.RATIO)
    own = [sc.voxel_map(P[w * lc.S:(w + 1) * lc.S], lc.VS, lc.RATIO, frame_begin=w * lc.S, n_frames=lc.S) for w in range(4)]
    yield dict(s=s, sc=sc, sm=sm, own=own, P=P)
    for m in own:
        m.close()
    sm.close()
    sc.close()


def relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_submap_lookup_equals_the_submaps_own_map(pkg, world):
    """7 frames in submaps of 3: 3 + 3 + 1 frames, the last ragged -- and, with one sparse cloud as its only frame, without a
    single plane.  Per submap the lookup gives the bytes of lvba_voxmap_find_planes on the map of those frames alone."""
    s, P = world["s"], world["P"]
    rng = np.random.default_rng(11)
    clouds = [c[:, :3] for c in s["clouds"][:6]] + [s["clouds"][6][:40, :3]]
    X = np.concatenate([ro.world_points(P[f], clouds[f][::7]) for f in range(7)] +
                       [rng.uniform(50.0, 60.0, (20, 3)), np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])])
    with pkg.Scans(clouds) as sc, sc.submaps(P[:7], 3, lc.VS, lc.RATIO) as sm:
        assert (sm.n_submaps, sm.submap_size) == (3, 3)
        planes = 0
        for w in range(3):
            fr = range(3 * w, min(3 * w + 3, 7))
            with sc.voxel_map(P[fr.start:fr.stop], lc.VS, lc.RATIO, frame_begin=fr.start, n_frames=len(fr)) as own:
                want, wv = own.find_planes(X)
                got, gv = sm.find_planes(X, w)
                print(f"submap {w}: {own.info['n_roots']} roots, {own.info['n_planes']} planes, {int(wv.sum())} of {len(X)} points on a plane")
                assert got.tobytes() == want.tobytes() and gv.tobytes() == wv.tobytes()
                assert (own.info["n_planes"] == 0) == (w == 2) and (wv.sum() > 100) == (w < 2)
                assert not wv[-22:].any()
                planes += own.info["n_planes"]
        assert sm.info["n_planes"] == planes
        # mixed indices in one call, out-of-range ones among them
        idx = (np.arange(len(X)) % 5 - 1).astype(np.int32)                  # -1, 0, 1, 2, 3
        got, gv = sm.find_planes(X, idx)
        for w in range(3):
            one, ov = sm.find_planes(X, w)
            assert got[idx == w].tobytes() == one[idx == w].tobytes() and gv[idx == w].tobytes() == ov[idx == w].tobytes()
        bad = (idx < 0) | (idx > 2)
        assert not gv[bad].any() and not got[bad].any() and gv[~bad].any()
        # the single-map calls keep refusing a set of several submaps
        L = pkg._lib
        with pytest.raises(L.LvbaError) as e:
            pkg.VoxelMap.find_planes(sm, X)
        assert e.value.code == L.ERR_UNSUPPORTED
        with pytest.raises(L.LvbaError) as e:
            pkg.VoxelMap.register(sm, sc, [0], P[:1])
        assert e.value.code == L.ERR_UNSUPPORTED


def check_lin(got, k, ref):
    fig = dict(inliers=(int(got["inliers"][k]), ref["inliers"]), H=relmax(got["H"][k], ref["H"]), g=relmax(got["g"][k], ref["g"]),
               cost=abs(got["cost"][k] - ref["cost"]) / ref["cost"])
    print("linearisation parity:", fig)
    assert got["inliers"][k] == ref["inliers"] and ref["inliers"] > 500
    assert fig["H"] <= 1e-11 and fig["g"] <= 1e-11 and fig["cost"] <= 1e-11


JOBS = [(0, 3), (10, 0), (1, 3), (10, 0), (11, 0), (5, 1)]                # (frame, submap); (10, 0) twice; (5, 1): its own submap


@pytest.mark.parametrize("loss", [None, ("cauchy", 0.03)])
def test_linearisation_per_submap(pkg, world, loss):
    sc, sm, P = world["sc"], world["sm"], world["P"]
    kw = dict(max_distance=lc.OPTS["max_distance"], **({} if loss is None else dict(loss=loss)))
    fr, w = [j[0] for j in JOBS], [j[1] for j in JOBS]
    got = sm.linearize(sc, fr, w, P[fr], **kw)
    for k, (f, v) in enumerate(JOBS):
        own = world["own"][v].register_linearize(sc, [f], P[f:f + 1], **kw)
        for key in ("H", "g", "cost", "inliers"):
            assert got[key][k].tobytes() == own[key][0].tobytes(), (key, f, v)
        alone = sm.linearize(sc, [f], [v], P[f:f + 1], **kw)
        assert alone["H"][0].tobytes() == got["H"][k].tobytes() and alone["g"][0].tobytes() == got["g"][k].tobytes()
    for key in ("H", "g", "cost", "inliers"):
        assert got[key][1].tobytes() == got[key][3].tobytes()
    for k in (0, 1):
        check_lin(got, k, lc.oracle_linearize("truth", fr[k], w[k], loss))
    if loss is None:   # a padded point stride: the same points, the same bytes
        rng = np.random.default_rng(2)
        padded = [np.concatenate([c[:, :3], rng.random((len(c), 1), dtype=np.float32)], 1) for c in world["s"]["clouds"]]
        with pkg.Scans(padded) as sp:
            gp = sm.linearize(sp, fr[:2], w[:2], P[fr[:2]], **kw)
        assert gp["H"].tobytes() == got["H"][:2].tobytes() and gp["cost"].tobytes() == got["cost"][:2].tobytes()


def test_iteration_per_submap(pkg, world):
    """From the drifted poses against submaps built at the drifted poses: every linearisation's inliers and cost and the final
    pose against the oracle, and the bytes of lvba_register_scans on the submap's own map."""
    sc = world["sc"]
    L = pkg._lib
    x = lc.drifted()
    cand = lc.candidates("drifted")
    fr, w = [c[0] for c in cand], [c[1] for c in cand]
    with sc.submaps(x, lc.S, lc.VS, lc.RATIO) as sm:
        full = sm.register(sc, fr, w, x[fr], **lc.OPTS)
        for k, (f, v) in enumerate(zip(fr, w)):
            ref = lc.oracle_register("drifted", f, v)
            with sc.voxel_map(x[v * lc.S:(v + 1) * lc.S], lc.VS, lc.RATIO, frame_begin=v * lc.S, n_frames=lc.S) as own:
                one = own.register(sc, [f], x[f:f + 1], **lc.OPTS)
            for key in ("poses", "information", "status", "iterations", "inliers", "cost_first", "cost_last", "rmse", "min_eigenvalue"):
                assert full[key][k].tobytes() == one[key][0].tobytes(), (key, f, v)
            assert full["status"][k] == ref["status"] == ro.CONVERGED and full["iterations"][k] == ref["iterations"]
            T = x[f]
            for it, t in enumerate(ref["trace"]):
                step = sm.register(sc, [f], [v], T[None], **dict(lc.OPTS, max_iterations=1))
                print(f"job ({f}, {v}) iteration {it}: inliers {step['inliers'][0]} / {t['inliers']}, cost {step['cost_last'][0]:.15e} / "
                      f"{t['cost']:.15e}, |pose - oracle| {np.abs(T - t['pose']).max():.2e}")
                assert step["inliers"][0] == t["inliers"] and abs(step["cost_last"][0] - t["cost"]) <= 1e-11 * t["cost"]
                assert np.abs(T - t["pose"]).max() <= 1e-7
                T = step["poses"][0]
            assert T.tobytes() == full["poses"][k].tobytes()
            assert np.abs(full["poses"][k] - ref["pose"]).max() <= 1e-7
        # a bad submap index, and the single-map calls on the set
        for bad in (-1, 4):
            with pytest.raises(L.LvbaError) as e:
                sm.register(sc, [0], [bad], x[:1], **lc.OPTS)
            assert e.value.code == L.ERR_ARG
        assert L.load().lvba_register_scans_submaps(sm._h, sc._h, 0, None, None, None, None, None, None, None) == L.OK
    # an empty submap: 7 frames in submaps of 3, the last a sparse cloud without a plane
    clouds = [c[:, :3] for c in world["s"]["clouds"][:6]] + [world["s"]["clouds"][6][:40, :3]]
    P = world["P"]
    with pkg.Scans(clouds) as s7, s7.submaps(P[:7], 3, lc.VS, lc.RATIO) as sm7:
        r = sm7.register(s7, [0, 0], [2, 0], P[[0, 0]], **lc.OPTS)
        assert r["status_name"][0] == "too_few_inliers" and r["inliers"][0] == 0 and r["poses"][0].tobytes() == P[0].tobytes()
        assert r["status_name"][1] == "converged"
    # a plain map is a set of one submap
    own = world["own"][0]
    a = own.register(sc, [10], P[10:11], **lc.OPTS)
    b = importlib.import_module("global-lvba_amd.register").register(own, sc, [10], P[10:11], submap=[0], **lc.OPTS)
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["information"].tobytes() == b["information"].tobytes()
    with pytest.raises(L.LvbaError) as e:
        importlib.import_module("global-lvba_amd.register").register(own, sc, [10], P[10:11], submap=[1], **lc.OPTS)
    assert e.value.code == L.ERR_ARG


def test_candidates_equal_the_oracle(pkg):
    reg = importlib.import_module("global-lvba_amd.register")
    L = pkg._lib
    for name, P, o in search_cases():
        want = lo.candidates(P, **o)
        got = reg.loop_candidates(P, **o)
        have = list(zip(got["query"].tolist(), got["submap"].tolist(), got["ref"].tolist(), got["distance"].tolist()))
        print(f"{name}: {got['count']} candidates")
        assert got["count"] == len(want) and have == want, name
        assert got["raw"].tobytes() == reg.loop_candidates(P, **o)["raw"].tobytes(), name     # two calls, the same bytes
        assert not got["raw"]["pad"].any()
    # a capacity below the count: the count stays true, nothing is written past the capacity
    P, o = lc.laps(), lc.LAPS_CASES[0]
    want = lo.candidates(P, **o)
    lib = L.load()
    opts = L.LoopOpts(**o)
    x = np.ascontiguousarray(P)
    for cap in (0, 5):
        buf = np.full(3 * (cap + 2), -7.0)
        n = C.c_int64()
        assert lib.lvba_loop_candidates(0, len(P), x.ctypes.data, C.byref(opts), cap, buf.ctypes.data, C.byref(n)) == L.OK
        assert n.value == len(want) > 5 and np.all(buf[3 * cap:] == -7.0)
        part = reg.loop_candidates(P, capacity=cap, **o)
        assert part["count"] == len(want) and list(part["query"]) == [c[0] for c in want[:cap]] and list(part["ref"]) == [c[2] for c in want[:cap]]
    # bad options and arguments
    for bad in (dict(submap_size=0), dict(min_gap=-1), dict(max_per_frame=0), dict(max_per_frame=33), dict(query_stride=0),
                dict(radius=0.0), dict(radius=np.inf), dict(radius=np.nan)):
        with pytest.raises(L.LvbaError) as e:
            reg.loop_candidates(P, **dict(o, **bad))
        assert e.value.code == L.ERR_ARG, bad
    nanp = P.copy()
    nanp[3, 10] = np.nan
    with pytest.raises(L.LvbaError) as e:
        reg.loop_candidates(nanp, **o)
    assert e.value.code == L.ERR_ARG
    n = C.c_int64()
    assert lib.lvba_loop_candidates(0, -1, x.ctypes.data, C.byref(opts), 0, None, C.byref(n)) == L.ERR_ARG
    assert lib.lvba_loop_candidates(0, len(P), x.ctypes.data, C.byref(opts), 4, None, C.byref(n)) == L.ERR_ARG
    assert lib.lvba_loop_candidates(0, len(P), x.ctypes.data, None, 0, None, C.byref(n)) == L.OK     # NULL options: the defaults


def test_find_loop_closures_end_to_end(pkg, world):
    """On the drifted fixture find_loop_closures accepts exactly what the oracle accepts, its priors are the shared helper's on the
    oracle's registrations, a start 1 m off is reported as rejected, and run_full_pipeline hands the priors to the LiDAR stage.
    Not asserted: that run_lidar_ba(priors=found) ends closer to poses_gt at the last frame than run_lidar_ba().  On this fixture
    the LiDAR stage alone removes most of the drift (start 26.2 mrad / 80.0 mm; without priors 6.5 mrad / 30.7 mm; with them
    15.4 mrad / 29.9 mm): every frame of the room sees every wall.  DESIGN.md §10d has the figures."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    sc = world["sc"]
    x = lc.drifted()
    kw = dict(submap_size=lc.S, voxel_size=lc.VS, radius=lc.RADIUS, min_gap=lc.MIN_GAP, **lc.ACCEPT, **lc.OPTS)
    priors, report = pl.find_loop_closures(sc, x, **kw)
    cand = lc.candidates("drifted")
    assert [(r["query"], r["submap"], r["ref"], r["distance"]) for r in report] == cand
    want = [lc.oracle_accept("drifted", q, w) for q, w, _, _ in cand]
    assert [(r["accepted"], r["reason"]) for r in report] == [(ok, why) for ok, why, _ in want]
    acc = [(c, reg) for c, (ok, _, reg) in zip(cand, want) if ok]
    assert len(priors) == len(acc) >= 2
    for p, ((q, w, ref, _), reg) in zip(priors, acc):
        o = pl.registration_prior(ref, q, x[ref], reg["pose"], reg["information"], reg["rmse"], reg["status"])
        fig = (relmax(p.meas[:], o.meas[:]), relmax(p.sqrt_info[:], o.sqrt_info[:]))
        print(f"prior ({ref}, {q}): measurement {fig[0]:.2e}, sqrt_info {fig[1]:.2e} from the oracle's")
        assert (p.i, p.j) == (ref, q) and fig[0] <= 1e-7 and fig[1] <= 1e-7
    # a tight bound on the correction rejects every candidate of the drifted start, with its reason
    _, tight = pl.find_loop_closures(sc, x, **dict(kw, max_trans=0.01))
    assert [lc.oracle_accept("drifted", q, w, max_trans=0.01)[:2] for q, w, _, _ in cand] == [(r["accepted"], r["reason"]) for r in tight]
    assert all(r["reason"] == "correction" for r in tight)
    # one candidate's start moved 1 m off: reported, rejected, the others as before
    off = x.copy()
    q0, w0 = cand[0][0], cand[0][1]
    off[q0, 9:] += np.array([0.0, 0.0, 1.0])                                # straight up: every distance within RADIUS stays so
    assert [c[:3] for c in lo.candidates(off, **lc.SEARCH)] == [c[:3] for c in cand]
    pr2, rep2 = pl.find_loop_closures(sc, off, **kw)
    ok, why, _ = lc.oracle_accept("drifted", q0, w0, start=off[q0])
    print("1 m off:", rep2[0]["status_name"], rep2[0]["inliers"], rep2[0]["rmse"], rep2[0]["trans"], rep2[0]["reason"], "oracle:", ok, why)
    assert not ok and (rep2[0]["accepted"], rep2[0]["reason"]) == (ok, why) and rep2[0]["query"] == q0
    assert q0 not in [p.j for p in pr2]
    # the whole pipeline: off by default, the report and the priors when asked for
    s = world["s"]
    clouds = [c[:, :3] for c in s["clouds"]]
    args = (clouds, x, np.arange(lc.N, dtype=np.float64), [], np.zeros((0, 12)), np.eye(3), np.zeros(3), None, 0, 0, [], [], [])
    cfg = dict(enable_visual_ba=False, window_size=3)
    plain = pl.run_full_pipeline(*args, **cfg)
    assert "loop_closures" not in plain and "priors_used" not in plain["lidar_report"]
    out = pl.run_full_pipeline(*args, loop_closures=kw, **cfg)
    assert [(r["query"], r["submap"], r["accepted"]) for r in out["loop_closures"]] == [(r["query"], r["submap"], r["accepted"]) for r in report]
    rep = out["lidar_report"]
    print("lidar report:", {k: rep[k] for k in ("n_anchors", "priors_used", "priors_dropped", "stage_ran")})
    assert rep["priors_used"] + rep["priors_dropped"] == len(priors)
