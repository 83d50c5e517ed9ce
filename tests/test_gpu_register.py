"""GPU tests of the scan-to-map registration (lvba_register_linearize / lvba_register_scans, VoxelMap.register,
pipeline.loop_closure_prior) against the numpy restatement (tests/register_oracle.py) on the shared fixture
(tests/register_cases.py): frames 0-4 of make_scans(6, 3000, room=(8, 6, 3)) are the map, frame 5 is registered."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

import register_cases as rc
import register_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg):
    s = rc.scans()
    sc = pkg.Scans(s["clouds"])
    m = sc.voxel_map(s["poses_gt"][:rc.MAP_FRAMES], rc.VS, rc.RATIO, n_frames=rc.MAP_FRAMES)
    yield dict(s=s, sc=sc, m=m)
    m.close()
    sc.close()


def relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def check_lin(got, k, ref, min_ref_inliers=500):
    """Inlier counts equal; H, g, cost to 1e-11 of their largest entry: a reordered fp64 sum of <= 3000 terms of like sign.
    min_ref_inliers: what the oracle itself must exceed for the case to mean something (a condition on the fixture)."""
    fig = dict(inliers=(int(got["inliers"][k]), ref["inliers"]), H=relmax(got["H"][k], ref["H"]), g=relmax(got["g"][k], ref["g"]),
               cost=abs(got["cost"][k] - ref["cost"]) / ref["cost"])
    print("linearisation parity:", fig)
    assert got["inliers"][k] == ref["inliers"] and ref["inliers"] > min_ref_inliers
    assert fig["H"] <= 1e-11 and fig["g"] <= 1e-11 and fig["cost"] <= 1e-11
    assert np.array_equal(got["H"][k], got["H"][k].T)


def test_linearisation_parity_batch_and_stride(pkg, world):
    """The truth, the perturbed start and the start again in one batch of three jobs on the same scan: each against the oracle,
    the two equal jobs byte for byte, and each equal to the job run alone (the sums depend on the job's own point count only)."""
    sc, m = world["sc"], world["m"]
    assert m.info["n_roots"] > 150 and m.info["n_planes"] > 100
    poses = np.stack([rc.start(), rc.truth(), rc.start()])
    got = m.register_linearize(sc, [rc.QUERY] * 3, poses, max_distance=rc.GATE)
    check_lin(got, 0, rc.oracle_linearize("start"))
    check_lin(got, 1, rc.oracle_linearize("truth"))
    for key in ("H", "g", "cost", "inliers"):
        assert got[key][0].tobytes() == got[key][2].tobytes()
    alone = m.register_linearize(sc, [rc.QUERY], poses[1:2], max_distance=rc.GATE)
    assert alone["H"][0].tobytes() == got["H"][1].tobytes() and alone["g"][0].tobytes() == got["g"][1].tobytes()
    # a padded point stride (x, y, z, payload): the same points, the same bytes
    rng = np.random.default_rng(2)
    padded = [np.concatenate([c[:, :3], rng.random((len(c), 1), dtype=np.float32)], 1) for c in world["s"]["clouds"]]
    with pkg.Scans(padded) as sp:
        gp = m.register_linearize(sp, [rc.QUERY], poses[:1], max_distance=rc.GATE)
    assert gp["H"][0].tobytes() == got["H"][0].tobytes() and gp["cost"][0] == got["cost"][0]


def test_linearisation_of_ragged_scans(pkg, world):
    """The query scan cut to 1, 63, 65 and 257 points -- one lane, a wavefront less one, a wavefront and one, a workgroup's 256
    lanes and one: each against the oracle, and byte for byte what the same job gives inside a batch with the full scan.  The
    oracle finds 1, 24, 24 and 113 inliers among them, so the fixture's bar of 500 becomes "at least one" here."""
    m, q, T = world["m"], rc.query_points(), rc.start()
    cuts = (1, 63, 65, 257)
    with pkg.Scans([q] + [q[:n] for n in cuts]) as sc:
        batch = m.register_linearize(sc, list(range(len(cuts) + 1)), np.tile(T, (len(cuts) + 1, 1)), max_distance=rc.GATE)
        check_lin(batch, 0, rc.oracle_linearize("start"))
        for k, n in enumerate(cuts, 1):
            alone = m.register_linearize(sc, [k], T[None], max_distance=rc.GATE)
            check_lin(alone, 0, ro.linearize(rc.oracle_map(), rc.VS, T, q[:n], rc.GATE), min_ref_inliers=0)
            for key in ("H", "g", "cost", "inliers"):
                assert alone[key][0].tobytes() == batch[key][k].tobytes(), (key, n)


def test_linearisation_parity_with_a_loss(world):
    ref = ro.linearize(rc.oracle_map(), rc.VS, rc.start(), rc.query_points(), rc.GATE, ("cauchy", 0.03))
    got = world["m"].register_linearize(world["sc"], [rc.QUERY], rc.start()[None], max_distance=rc.GATE, loss=("cauchy", 0.03))
    check_lin(got, 0, ref)


def test_iteration_parity_and_convergence(world):
    """Every iteration's inlier count and cost and the final pose against the oracle.  All of the oracle's iterations have a decision
    margin above 1e-9 m on this fixture (seed 5; asserted), so all are compared.  Per-iteration figures: the run is cut into single
    iterations, each starting from the last one's pose, which is the same arithmetic as one run and must give its bytes."""
    sc, m = world["sc"], world["m"]
    ref = rc.oracle_register()
    assert all(t["margin"] > 1e-9 for t in ref["trace"]) and ref["status"] == ro.CONVERGED
    full = m.register(sc, [rc.QUERY], rc.start()[None], **rc.OPTS)
    print("registration:", {k: full[k][0] for k in ("status", "iterations", "inliers", "cost_first", "cost_last", "rmse", "min_eigenvalue")})
    assert full["status"][0] == ref["status"] and full["iterations"][0] == ref["iterations"] and full["points"][0] == 3000
    T = rc.start()
    for k, t in enumerate(ref["trace"]):
        one = m.register(sc, [rc.QUERY], T[None], **dict(rc.OPTS, max_iterations=1))
        print(f"iteration {k}: inliers {one['inliers'][0]} / {t['inliers']}, cost {one['cost_last'][0]:.15e} / {t['cost']:.15e}, "
              f"margin {t['margin']:.2e}, |pose - oracle| {np.abs(T - t['pose']).max():.2e}")
        assert one["inliers"][0] == t["inliers"]
        assert abs(one["cost_last"][0] - t["cost"]) <= 1e-11 * t["cost"]
        assert np.abs(T - t["pose"]).max() <= 1e-7
        T = one["poses"][0]
    assert T.tobytes() == full["poses"][0].tobytes()
    assert np.abs(full["poses"][0] - ref["pose"]).max() <= 1e-7
    assert full["inliers"][0] == ref["inliers"]
    assert abs(full["cost_first"][0] - ref["cost_first"]) <= 1e-11 * ref["cost_first"]
    assert relmax(full["information"][0], ref["information"]) <= 1e-9       # H at the last pose, itself at 1e-7 of the oracle's
    assert abs(full["min_eigenvalue"][0] - ref["min_eigenvalue"]) <= 1e-9
    # convergence: closer to the truth than the start, rmse as the oracle's
    a0, d0 = ro.pose_error(rc.start(), rc.truth())
    a1, d1 = ro.pose_error(full["poses"][0], rc.truth())
    assert a1 < a0 and d1 < d0 and a1 <= 1e-3 and d1 <= 5e-3
    assert abs(full["rmse"][0] - ref["rmse"]) <= 1e-9


def test_status_paths_and_reproducibility(pkg, world):
    sc, m = world["sc"], world["m"]
    L = pkg._lib
    T = rc.start()[None]
    # two runs, a batch of two equal jobs: the same bytes
    a = m.register(sc, [rc.QUERY, rc.QUERY], np.concatenate([T, T]), **rc.OPTS)
    b = m.register(sc, [rc.QUERY, rc.QUERY], np.concatenate([T, T]), **rc.OPTS)
    for key in ("poses", "information", "cost_last", "rmse", "min_eigenvalue", "inliers", "iterations"):
        assert a[key].tobytes() == b[key].tobytes() and a[key][0].tobytes() == a[key][1].tobytes()
    # a gate so small that too few points remain
    r = m.register(sc, [rc.QUERY], T, **dict(rc.OPTS, max_distance=1e-7))
    assert r["status_name"] == ["too_few_inliers"] and r["iterations"][0] == 1 and r["inliers"][0] < 100
    assert r["poses"][0].tobytes() == T[0].tobytes()
    # an empty map: not an error
    with pkg.VoxelMap([np.zeros((0, 3), np.float32)], np.r_[np.eye(3).reshape(9), np.zeros(3)][None]) as empty:
        r = empty.register(sc, [0, rc.QUERY], np.concatenate([T, T]), **rc.OPTS)
    assert r["status_name"] == ["too_few_inliers"] * 2 and list(r["inliers"]) == [0, 0] and r["poses"].tobytes() == np.concatenate([T, T]).tobytes()
    # a map of one single plane: degenerate, pose unchanged
    rng = np.random.default_rng(3)
    flat = [np.c_[rng.uniform(0.2, 3.8, (2000, 2)), 1e-3 * rng.standard_normal(2000)].astype(np.float32) for _ in range(2)]
    I = np.tile(np.r_[np.eye(3).reshape(9), 0.0, 0.0, 0.5], (2, 1))
    with pkg.Scans(flat) as fs, fs.voxel_map(I, 1.0, rc.RATIO) as fm:
        r = fm.register(fs, [1], I[1:], **rc.OPTS)
        assert r["status_name"] == ["degenerate"] and r["inliers"][0] > 1500 and abs(r["min_eigenvalue"][0]) < 1e-6
        assert r["poses"][0].tobytes() == I[1].tobytes()
    # argument errors
    for frames, poses, kw in (([6], T, {}), ([-1], T, {}), ([rc.QUERY], np.full((1, 12), np.nan), {}),
                              ([rc.QUERY], T, dict(max_distance=0.0)), ([rc.QUERY], T, dict(loss=("huber", -1.0)))):
        with pytest.raises(L.LvbaError) as e:
            m.register(sc, frames, poses, **kw)
        assert e.value.code == L.ERR_ARG
    lib = L.load()
    assert lib.lvba_register_scans(m._h, sc._h, -1, None, None, None, None, None, None) == L.ERR_ARG
    assert lib.lvba_register_scans(m._h, sc._h, 0, None, None, None, None, None, None) == L.OK


def test_joint_map_is_refused(pkg, world):
    """A joint map of several windows and a view into one have no key lookup: LVBA_ERR_UNSUPPORTED, as find_planes.  Such maps
    are made by the window driver only; the test reaches its two internal builders through their C++ names."""
    L = pkg._lib
    lib = L.load()
    names = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True).split()
    build = next(n for n in names if "lvba_voxmap_build_scans_joint" in n)
    view = next(n for n in names if "lvba_voxmap_window_view" in n)
    fb, fv = getattr(lib, build), getattr(lib, view)
    fb.restype = fv.restype = C.c_int32
    fb.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    fv.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    sc = world["sc"]
    poses = np.ascontiguousarray(world["s"]["poses_gt"], np.float64)
    o = importlib.import_module("global-lvba_amd.voxel")._opts(rc.VS, rc.RATIO, None)
    joint, v = C.c_void_p(), C.c_void_p()
    assert fb(sc._h, 0, 6, 3, poses.ctypes.data, C.addressof(o), None, C.byref(joint)) == L.OK
    try:
        assert fv(joint, 1, C.byref(v)) == L.OK
        T = np.ascontiguousarray(rc.start())
        fr = np.array([rc.QUERY], np.int32)
        out, info, res = np.zeros(12), np.zeros(36), L.RegisterResult()
        for h in (joint, v):
            assert lib.lvba_register_scans(h, sc._h, 1, fr.ctypes.data, T.ctypes.data, None, out.ctypes.data, info.ctypes.data,
                                           C.addressof(res)) == L.ERR_UNSUPPORTED
            assert lib.lvba_register_linearize(h, sc._h, 1, fr.ctypes.data, T.ctypes.data, None, info.ctypes.data, out.ctypes.data,
                                               out.ctypes.data, fr.ctypes.data) == L.ERR_UNSUPPORTED
    finally:
        if v.value:
            lib.lvba_voxmap_destroy(v)
        lib.lvba_voxmap_destroy(joint)


def test_loop_closure_prior(pkg, world):
    """frames 0-4 at the truth, frame 5 from the perturbed start: the prior between frame 0 and frame 5 has a zero residual at
    the registered pose, and its information is the registration's in the prior's tangent."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    sc = world["sc"]
    poses = world["s"]["poses_gt"].copy()
    poses[rc.QUERY] = rc.start()
    prior, reg = pl.loop_closure_prior(sc, poses, range(rc.MAP_FRAMES), rc.QUERY, voxel_size=rc.VS, **rc.OPTS)
    ref = rc.oracle_register()
    assert reg["status"][0] == 0 and np.abs(reg["poses"][0] - ref["pose"]).max() <= 1e-7
    assert prior.i == 0 and prior.j == rc.QUERY
    Lm = np.array(prior.sqrt_info[:]).reshape(6, 6)
    R0 = poses[0, :9].reshape(3, 3)
    M = np.zeros((6, 6))
    M[:3, :3], M[3:, 3:] = np.eye(3), R0.T
    assert relmax(Lm.T @ Lm, M @ reg["information"][0] @ M.T / reg["rmse"][0] ** 2) <= 1e-12
    x = poses.copy()
    x[rc.QUERY] = reg["poses"][0]
    with sc.voxel_map(x, rc.VS, rc.RATIO) as m6, m6.tras_opt() as prob:
        prob.set_priors([prior])
        e, c = prob.prior_residuals(x)
        print("prior residual at the registered pose:", np.abs(e).max())
        assert np.abs(e).max() <= 1e-9
        e0, _ = prob.prior_residuals(poses)                                 # at the start it pulls: 0.1 m / 6 mm
        assert np.abs(e0).max() > 1.0
