"""GPU tests of the pose-graph relaxation: lvba_posegraph_relax against the numpy oracle (tests/posegraph_oracle.py) on the shared
cases (tests/posegraph_cases.py), its argument checks, and pipeline.relax_trajectory / run_full_pipeline(relax=...) on the fixtures
of §10d and §10e."""
import ctypes as C
import importlib

import numpy as np
import pytest

import loop_cases as lc
import place_cases as pc
import posegraph_cases as pgc
import posegraph_oracle as pg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pgm(pkg):
    return importlib.import_module("global-lvba_amd.posegraph")


@pytest.fixture(scope="module")
def pl(pkg):
    return importlib.import_module("global-lvba_amd.pipeline")


def priors_of(closures):
    balm = importlib.import_module("global-lvba_amd.balm")
    return [balm.Prior.relative(p["i"], p["j"], p["meas"], sqrt_info=p["L"], offset_i=p["oi"], offset_j=p["oj"]) for p in closures]


def run(pgm, c, closures=None, **more):
    return pgm.relax_pose_graph(c["X"], priors_of(c["closures"] if closures is None else closures), **dict(c["opts"], **more))


@pytest.mark.parametrize("N", [2, 3])
def test_no_closures_returns_the_input(pgm, N):
    X = pgc.ring(8)[:N]
    got = pgm.relax_pose_graph(X, [])
    assert got["poses"].tobytes() == X.tobytes() and got["trace"] == [] and len(got["weights"]) == 0
    r = got["report"]
    assert (r["iterations"], r["accepted"], r["status"], r["cost_first"], r["cost_last"], r["solver"]) == (0, 0, 0, 0.0, 0.0, "none")


@pytest.mark.parametrize("name", pgc.names())
def test_relaxation_equals_the_oracle(pgm, monkeypatch, name):
    """Poses within posegraph_cases.POSE_TOL of the oracle's (rotation angle and position separately), the same accept / reject
    sequence, the costs and the weights to 1e-9 relative, the solver the case is meant to reach, two calls bitwise equal, and the
    result unchanged (to POSE_TOL) under a permutation of the edge array."""
    c = pgc.named(name)
    if c["env"]:
        monkeypatch.setenv("LVBA_SOLVER", c["env"])
    want = pgc.oracle(name)
    got = run(pgm, c)
    rot, pos = pg.pose_errors(got["poses"], want["poses"])
    r, w = got["report"], want["report"]
    seq = lambda t: [(x["accepted"], x["evaluated"]) for x in t]
    print(f"{name}: solver {r['solver']}, {r['iterations']} iterations, cost {r['cost_first']:.6g} -> {r['cost_last']:.6g}, "
          f"|poses - oracle| {rot:.2e} rad {pos:.2e} m, cost_last rel {abs(r['cost_last'] - w['cost_last']) / w['cost_last']:.2e}")
    assert r["status"] == 0 and seq(got["trace"]) == seq(want["trace"]) and r["iterations"] == w["iterations"] and r["accepted"] == w["accepted"]
    if c["solver"]:
        assert r["solver"] == c["solver"]
    assert rot <= pgc.POSE_TOL["rot"] and pos <= pgc.POSE_TOL["pos"]
    for f in ("cost_first", "cost_last", "odom_cost_last", "closure_cost_last"):
        assert abs(r[f] - w[f]) <= 1e-9 * abs(w[f]), f
    # a step is the difference of two pose sets that are each within POSE_TOL of the oracle's
    assert abs(r["max_step_last"] - w["max_step_last"]) <= 2.0 * max(pgc.POSE_TOL.values())
    assert np.abs(got["weights"] - want["weights"]).max() <= 1e-9
    again = run(pgm, c)
    assert again["poses"].tobytes() == got["poses"].tobytes() and again["weights"].tobytes() == got["weights"].tobytes()
    assert again["trace"] == got["trace"] and again["report"] == got["report"]
    if len(c["closures"]) > 1:
        perm = np.random.default_rng(5).permutation(len(c["closures"]))
        other = run(pgm, c, closures=[c["closures"][k] for k in perm])
        rot2, pos2 = pg.pose_errors(other["poses"], got["poses"])
        print(f"  permuted edges: {rot2:.2e} rad {pos2:.2e} m")
        assert rot2 <= pgc.POSE_TOL["rot"] and pos2 <= pgc.POSE_TOL["pos"]
        assert np.abs(other["weights"] - got["weights"][perm]).max() <= 1e-9


def test_pair_minimum_in_closed_form(pgm):
    """N = 2, the closure says the odometry's rotation and a translation d farther, with the odometry's information: the relative
    translation ends at the midpoint, the rotation does not change, pose 0 stays."""
    c = pgc.named("pair")
    got = run(pgm, c, rel_tol=1e-12)
    z0, zc = pg.relative(c["X"][0], c["X"][1]), c["closures"][0]["meas"]
    z = pg.relative(got["poses"][0], got["poses"][1])
    assert np.abs(got["poses"][0] - c["X"][0]).max() <= 1e-9
    assert np.abs(z[:9] - z0[:9]).max() <= 1e-9 and np.abs(z[9:] - 0.5 * (z0[9:] + zc[9:])).max() <= 1e-9


def test_cauchy_separates_the_false_closure(pgm):
    got = run(pgm, pgc.named("cauchy"))
    w = got["weights"]
    print("weights:", np.round(w, 4))
    assert w[-1] < 0.05 and w[:-1].min() > 0.95


def test_null_outputs_and_bad_arguments(pkg, pgm):
    L = pkg._lib
    lib = L.load()
    c = pgc.named("two laps")
    want = run(pgm, c)
    X = c["X"].copy()
    pri = priors_of(c["closures"])
    K, N = len(pri), len(X)
    o = pgm.posegraph_opts(**c["opts"])
    d = L.PosegraphOpts()
    lib.lvba_posegraph_default_opts(C.byref(d))
    assert (d.anchor, d.max_iter, d.odom_sigma_rot, d.odom_sigma_pos, d.anchor_sigma_rot, d.anchor_sigma_pos, d.rel_tol, d.closure_loss.kind) == \
        tuple(pg.DEFAULTS[k] for k in ("anchor", "max_iter", "odom_sigma_rot", "odom_sigma_pos", "anchor_sigma_rot", "anchor_sigma_pos", "rel_tol")) + (0,)

    def call(x=X, edges=pri, opts=o, n_poses=None, n_edges=None, null=False):
        arr = (L.Prior * max(1, len(edges)))(*edges)
        out, w = np.full((N, 12), -7.0), np.full(K, -7.0)
        trace, n_trace, rep = (L.LmTrace * 64)(), C.c_int32(-7), L.PosegraphReport(-7, -7, -7, -7, -7.0, -7.0, -7.0, -7.0, -7.0)
        rc = lib.lvba_posegraph_relax(N if n_poses is None else n_poses, x.ctypes.data, len(edges) if n_edges is None else n_edges,
                                      C.cast(arr, C.c_void_p), C.byref(opts), 0, out.ctypes.data, None if null else w.ctypes.data,
                                      None if null else C.cast(trace, C.c_void_p), None if null else C.byref(n_trace), C.byref(rep))
        return rc, out, w, n_trace.value, rep

    rc, out, w, n_trace, rep = call(null=True)      # NULL weights, trace and n_trace
    assert rc == L.OK and out.tobytes() == want["poses"].tobytes() and (w == -7.0).all() and n_trace == -7
    assert rep.as_dict() == {k: v for k, v in want["report"].items() if k != "solver"}

    def refused(**kw):
        rc, out, w, n_trace, rep = call(**kw)
        assert rc == L.ERR_ARG, kw
        assert (out == -7.0).all() and (w == -7.0).all() and n_trace == -7 and rep.iterations == -7 and rep.cost_last == -7.0

    def edit(k, **f):
        e = [L.Prior.from_buffer_copy(bytes(p)) for p in pri]
        for a, b in f.items():
            if isinstance(b, tuple):
                getattr(e[k], a)[b[0]] = b[1]
            else:
                setattr(e[k], a, b)
        return e

    refused(edges=edit(3, kind=0))                       # not RELATIVE
    refused(edges=edit(3, kind=1))
    refused(edges=edit(0, i=N))                          # index out of range
    refused(edges=edit(0, j=-1))
    refused(edges=edit(K - 1, j=pri[K - 1].i))           # i == j
    refused(edges=edit(2, meas=(9, float("nan"))))       # non-finite
    refused(edges=edit(2, sqrt_info=(7, float("inf"))))
    refused(edges=edit(2, meas=(0, 1.5)))                # not orthonormal
    refused(edges=edit(2, offset_j=(0, 0.5)))
    bad = X.copy(); bad[5, 10] = np.nan
    refused(x=bad)
    bad = X.copy(); bad[5, 0] += 0.1
    refused(x=bad)
    for f, v in (("odom_sigma_rot", 0.0), ("odom_sigma_pos", -1.0), ("anchor_sigma_rot", float("inf")), ("anchor_sigma_pos", float("nan")),
                 ("rel_tol", 0.0), ("max_iter", -1), ("anchor", N), ("anchor", -1)):
        refused(opts=pgm.posegraph_opts(**dict(c["opts"], **{f: v})))
    refused(opts=pgm.posegraph_opts(closure_loss=(9, 1.0)))
    refused(opts=pgm.posegraph_opts(closure_loss=("cauchy", 0.0)))
    refused(n_poses=1)
    refused(n_edges=-1)
    with pytest.raises(TypeError):
        pgm.relax_pose_graph(X, pri, radius=1.0)


def test_relaxation_brings_the_drifted_lap_within_the_pose_radius(pkg, pl):
    """The point of the stage, on §10e's fixture: at the drifted poses the pose search finds no revisit between the laps and the
    descriptor search (vetted) does; after relax_trajectory over those closures the largest lap-to-lap position error -- the offset
    of frame 12 + k from frame k against the same offset at the truth; the anchor, frame 0, is at the truth -- is below the pose
    radius, and the pose search finds revisits.
    The fixture's drift is ONE step of 9 m and 10 degrees (frame 11 -> 12) in an odometry that is otherwise exact.  Least squares
    cannot know which step is wrong: it closes the loop by spreading that step over the twelve steps of a lap, so both laps end
    deformed alike (by up to 8.03 m against the truth at frame 11 / 23, oracle and device) while lying on one another to
    millimetres.  That is what the bundle adjustment needs -- shared voxels -- and what this test asserts; the absolute error is
    printed, not asserted."""
    x, P = pc.drifted(), pc.truth()
    shared = {k: pc.PLACE[k] for k in ("submap_size", "min_gap", "max_per_frame")}
    place = {k: v for k, v in pc.PLACE.items() if k not in shared}
    reg = dict(voxel_size=lc.VS, **shared, **pc.ACCEPT, **pc.REG)
    with pkg.Scans(pc.clouds()) as sc:
        by_pose, _ = pl.find_loop_closures(sc, x, method="pose", radius=pc.POSE_RADIUS, **reg)
        found, _ = pl.find_loop_closures(sc, x, method="descriptor", place=place, consistency=True, **reg)
        assert by_pose == [] and len(found) >= 3
        got = pl.relax_trajectory(x, found)
        y = got["poses"]
        assert np.array_equal(y[0], x[0]) or np.abs(y[0] - x[0]).max() < 1e-9       # the anchor (frame 0 is at the truth)
        n = pc.N_LAP
        lap_to_lap = lambda z: np.linalg.norm((z[n:, 9:] - z[:n, 9:]) - (P[n:, 9:] - P[:n, 9:]), axis=1).max()
        before, after = lap_to_lap(x), lap_to_lap(y)
        print(f"{len(found)} closures, {got['report']['iterations']} iterations ({got['report']['solver']}), lap-to-lap position error "
              f"{before:.3f} m -> {after:.4f} m (radius {pc.POSE_RADIUS}); against the truth {np.linalg.norm(x[n:, 9:] - P[n:, 9:], axis=1).max():.3f}"
              f" -> {np.linalg.norm(y[:, 9:] - P[:, 9:], axis=1).max():.3f} m; largest pose change {got['max_pose_change']}")
        assert before > pc.POSE_RADIUS and after < pc.POSE_RADIUS
        again, _ = pl.find_loop_closures(sc, y, method="pose", radius=pc.POSE_RADIUS, **reg)
        assert len(again) >= 1 and all(p.j >= pc.N_LAP > p.i or p.i >= pc.N_LAP > p.j for p in again)


def test_pipeline_relax_is_opt_in(pkg, pl, tmp_path):
    """run_full_pipeline(loop_closures=..., relax=True) on §10d's fixture completes and reports the relaxation; relax=None returns
    what the call without the keyword returns, key for key and byte for byte."""
    s = lc.scans()
    x = lc.drifted()
    kw = dict(submap_size=lc.S, voxel_size=lc.VS, radius=lc.RADIUS, min_gap=lc.MIN_GAP, **lc.ACCEPT, **lc.OPTS)
    args = ([c[:, :3] for c in s["clouds"]], x, np.arange(lc.N, dtype=np.float64), [], np.zeros((0, 12)), np.eye(3), np.zeros(3), None, 0, 0,
            [], [], [])
    cfg = dict(enable_visual_ba=False, window_size=3)
    base = pl.run_full_pipeline(*args, loop_closures=kw, **cfg)
    none = pl.run_full_pipeline(*args, loop_closures=kw, relax=None, **cfg)
    alone = pl.run_full_pipeline(*args, relax=True, **cfg)             # without loop_closures the keyword does nothing
    assert "pose_graph" not in none and "pose_graph" not in alone and "loop_closures" not in alone

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), k
            elif k == "loop_closures":
                assert len(a[k]) == len(b[k]) and all(p["pose"].tobytes() == q["pose"].tobytes() and p["accepted"] == q["accepted"] for p, q in zip(a[k], b[k]))
            elif k == "lidar_report":
                keep = lambda r: {f: v for f, v in r.items() if f != "anchor_priors" and not f.endswith("_ms")}    # (timings differ)
                assert keep(a[k]) == keep(b[k])
            else:
                assert a[k] == b[k], k

    same(base, none)
    out = pl.run_full_pipeline(*args, loop_closures=kw, relax=dict(max_iter=20), **cfg)
    g = out["pose_graph"]
    print("pose graph:", g["report"], g["max_pose_change"])
    assert g["report"]["status"] == 0 and g["report"]["iterations"] >= 1 and g["report"]["cost_last"] < g["report"]["cost_first"]
    assert len(g["weights"]) == sum(1 for r in out["loop_closures"] if r["accepted"]) and out["poses"].shape == x.shape
    assert np.isfinite(out["poses"]).all() and out["poses_before"].tobytes() == x.tobytes()
