"""GPU tests of the pose priors of the LiDAR bundle adjustment (lvba_balm_set_priors): cost, H, g and the LM against the numpy model
of tests/prior_oracle.py on top of the C oracle, the pose graph the relative priors add to the store, gauge and GNSS use,
determinism over runs and ranks, the no-prior guard, and every refusal."""
import numpy as np
import pytest

import prior_oracle as po
from conftest import HostTransport, make_problem, rel

pytestmark = pytest.mark.gpu

BAND = dict(n_poses=150, n_voxels=8000, band=12, seed=4)
ND = dict(n_poses=320, n_voxels=16000, band=12, seed=3, revisit="lot")    # a hub: LVBA_SOLVER=nd dissects it
RANKS = dict(n_poses=200, n_voxels=6000, band=10, seed=7)
CHAIN = dict(n_poses=200, n_voxels=6000, band=5, seed=7, loop_frac=0.0)


def _c(pkg, pr):
    """oracle prior dict -> lvba_prior"""
    return pkg.Prior._make({0: "pose", 1: "position", 2: "relative"}[pr["kind"]], pr["i"], pr["j"], pr["meas"], pr["L"], pr["oi"], pr["oj"])


def _rel_gt(x, i, j):
    Ri, pi_ = x[i, :9].reshape(3, 3), x[i, 9:]
    Rj, pj = x[j, :9].reshape(3, 3), x[j, 9:]
    return np.r_[(Ri.T @ Rj).reshape(9), Ri.T @ (pj - pi_)]


def _mix(d, seed=0, loop=True):
    """POSE on pose 0, POSITION with a lever arm on every 10th pose, RELATIVE on every 7th consecutive pair and, with loop, one
    joining the two ends -- measurements from the ground truth with noise, so that they pull against the voxels"""
    rng = np.random.default_rng(seed)
    x = d["poses_gt"].reshape(-1, 12)
    N = x.shape[0]
    L6 = np.diag([40.0, 30.0, 20.0, 6.0, 4.0, 2.0])
    L6[4, 1] = 1.0
    R0 = x[0, :9].reshape(3, 3) @ po.so3_exp(rng.normal(scale=1e-3, size=3))
    out = [po.make_prior("pose", 0, np.r_[R0.reshape(9), x[0, 9:] + rng.normal(scale=0.01, size=3)], L6,
                         oi=np.r_[po.so3_exp([0.1, 0.2, -0.1]).reshape(9), 0.2, -0.1, 0.4])]
    arm = np.array([0.3, -0.1, 1.2])
    for i in range(0, N, 10):
        z = x[i, :9].reshape(3, 3) @ arm + x[i, 9:] + rng.normal(scale=0.01, size=3)
        out.append(po.make_prior("position", i, np.r_[np.eye(3).reshape(9), z], np.diag([5.0, 5.0, 3.0, 0, 0, 0]),
                                 oi=np.r_[np.eye(3).reshape(9), arm]))
    for i in range(1, N - 1, 7):
        a, b = (i + 1, i) if i % 2 else (i, i + 1)      # both orientations of the pair
        m = _rel_gt(x, a, b)
        m[:9] = (m[:9].reshape(3, 3) @ po.so3_exp(rng.normal(scale=1e-3, size=3))).reshape(9)
        m[9:] += rng.normal(scale=0.005, size=3)
        out.append(po.make_prior("relative", a, m, L6, j=b))
    if loop:
        out.append(po.make_prior("relative", N - 1, _rel_gt(x, N - 1, 0), L6, j=0,
                                 oi=np.r_[po.so3_exp([0.0, 0.3, 0.0]).reshape(9), 0.0, 0.5, 0.0],
                                 oj=np.r_[po.so3_exp([0.0, 0.3, 0.0]).reshape(9), 0.0, 0.5, 0.0]))
    return out


def _prob(pkg, d, priors=None, **kw):
    p = pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"], **kw)
    if priors is not None:
        p.set_priors([_c(pkg, q) for q in priors])
    return p


def _forms(monkeypatch, form):
    if form == "nd":
        monkeypatch.setenv("LVBA_SOLVER", "nd")
        return ND, {}
    if form == "dense":
        return BAND, dict(band_frac=0.0)
    return BAND, {}


@pytest.mark.parametrize("form", ["band", "dense", "nd"])
def test_cost_eval_and_residuals_match_the_oracle(pkg, oracle_mod, monkeypatch, form):
    case, kw = _forms(monkeypatch, form)
    d = make_problem(**case)
    priors = _mix(d)
    p = _prob(pkg, d, priors, **kw)
    if form == "nd":
        assert p.info()["nd_arcs"] >= 1
    if form == "dense":
        assert p.info()["use_band"] == 0
    orc = po.PriorOracle(oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]), priors)
    x = d["poses_init"]
    Hc, gc, cc = orc.eval_dense(x)
    H, g, c = p.eval(x)
    V = p.n_voxels
    assert abs(c * V - cc) <= 1e-9 * cc
    assert rel(g, gc) <= 1e-9 and rel(H, Hc) <= 1e-9 and np.array_equal(H, H.T)
    assert abs(p.cost(x) - orc.cost(x)) <= 1e-9 * orc.cost(x)
    assert abs(p.cost(x, is_avg=True) - orc.cost(x) / V) <= 1e-9 * orc.cost(x) / V
    e, ce = p.prior_residuals(x)
    ref = [po.residual(q, x) for q in priors]
    assert e.shape == (len(priors), 6)
    assert rel(e, np.stack([r[0] for r in ref])) <= 1e-9 and abs(ce - sum(r[1] for r in ref)) <= 1e-9 * ce
    # the prior terms alone: the difference to a handle without priors is the model's H, g, cost
    q = _prob(pkg, d, None, **kw)
    H0, g0, c0 = q.eval(x)
    Hp, gp, cp = po.assemble(priors, x)
    assert rel(H - H0, Hp) <= 1e-7 and rel(g - g0, gp) <= 1e-7 and abs((c - c0) * V - cp) <= 1e-7 * cp


def _compare(trace, tr_ref, x_gpu, x_ref, tol=1e-7):
    """Row by row, as tests/test_gpu_balm.py::_compare_traces, with the oracle's LMTraceRow fields."""
    tie = None
    for i, (row, ref) in enumerate(zip(trace, tr_ref)):
        if abs(ref.q) <= 3e-8 * abs(ref.residual1) or abs(row["q"]) <= 3e-8 * abs(row["residual1"]):
            tie = i
            break
        assert row["accepted"] == int(ref.accepted) and row["evaluated"] == int(ref.evaluated)
        assert abs(row["residual1"] - ref.residual1) <= tol * abs(ref.residual1)
        assert abs(row["residual2"] - ref.residual2) <= tol * abs(ref.residual2)
        assert abs(row["u"] - ref.u) <= 1e-4 * abs(ref.u)
    if tie is None:
        assert len(trace) == len(tr_ref)
        assert np.abs(x_gpu - x_ref).max() <= tol
    else:
        best = min(r["residual2"] if r["accepted"] else r["residual1"] for r in trace)
        best_ref = min(r.residual2 if r.accepted else r.residual1 for r in tr_ref)
        assert abs(best - best_ref) <= tol * best_ref
        assert np.abs(x_gpu - x_ref).max() <= 1e-5


@pytest.mark.parametrize("form", ["band", "nd"])
def test_lm_trace_matches_the_prior_oracle(pkg, oracle_mod, monkeypatch, form):
    case, kw = _forms(monkeypatch, form)
    if form == "band":                                # a band store (BAND's 900 unknowns are solved dense)
        monkeypatch.setenv("LVBA_SOLVER", "nond")
        case = RANKS
    d = make_problem(**case)
    priors = _mix(d, seed=1)
    p = _prob(pkg, d, priors, **kw)
    assert p.info()["use_band"] == (1 if form == "band" else 0)
    x, trace, rc = p.refine(d["poses_init"])
    assert rc == 0
    orc = po.PriorOracle(oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]), priors)
    xr, tr = orc.damping_iter(d["poses_init"])
    assert len(tr) >= 3
    _compare(trace, tr, x, xr)


def test_loop_closure_prior_folds_an_open_chain(pkg, oracle_mod, monkeypatch):
    monkeypatch.setenv("LVBA_SOLVER", "nond")
    d = make_problem(**CHAIN)
    N = d["n_poses"]
    x = d["poses_gt"].reshape(-1, 12)
    loop = [po.make_prior("relative", 0, _rel_gt(x, 0, N - 1), np.diag([100.0, 100, 100, 10, 10, 10]), j=N - 1)]
    bare = _prob(pkg, d)
    b0 = bare.info()["band_blocks"]
    assert b0 < 12
    p = _prob(pkg, d, loop)
    info = p.info()
    assert info["use_band"] == 1 and b0 < info["band_blocks"] <= 2 * b0 + 2               # a folded ring
    bi, bj, blocks, g, c = p.eval_blocks(d["poses_init"])
    k = np.nonzero((bi == N - 1) & (bj == 0))[0]
    assert k.size == 1 and np.abs(blocks[k[0]]).max() > 0                              # the block exists and holds the prior
    nat = _prob(pkg, d, loop, ordering=0)
    assert nat.info()["band_blocks"] == N - 1
    orc = po.PriorOracle(oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"]), loop)
    xr, tr = orc.damping_iter(d["poses_init"])
    for q in (p, nat):
        xg, trace, rc = q.refine(d["poses_init"])
        assert rc == 0
        _compare(trace, tr, xg, xr)
    Hd, _, _ = nat.eval(d["poses_init"])
    assert np.abs(Hd[6 * (N - 1):, :6]).max() > 0


def test_stiff_pose_prior_fixes_the_gauge(pkg):
    d = make_problem(n_poses=40, n_voxels=3000, band=10, seed=2)
    x0 = d["poses_init"].reshape(-1, 12)
    fix = po.make_prior("pose", 0, x0[0], 1e7 * np.eye(6))
    p = _prob(pkg, d, [fix])
    x, trace, rc = p.refine(x0)
    assert rc == 0 and len(trace) >= 2
    assert np.abs(x[0] - x0[0]).max() <= 1e-9
    free, _, _ = _prob(pkg, d).refine(x0)
    assert np.abs(free[0] - x0[0]).max() > 1e-7                                         # without it pose 0 moves


def test_gnss_position_priors_remove_a_planted_offset(pkg):
    d = make_problem(n_poses=40, n_voxels=3000, band=10, seed=2)
    gt = d["poses_gt"].reshape(-1, 12)
    x0 = d["poses_init"].reshape(-1, 12).copy()
    Rg = po.so3_exp([0.0, 0.0, 0.02])
    for i in range(len(x0)):                                      # a global rigid motion: the voxel cost cannot see it
        x0[i, :9] = (Rg @ x0[i, :9].reshape(3, 3)).reshape(9)
        x0[i, 9:] = Rg @ x0[i, 9:] + np.array([0.8, -0.5, 0.3])
    rng = np.random.default_rng(5)
    arm = np.array([0.2, 0.0, 1.5])
    fixes = [pkg.Prior.position(i, gt[i, :9].reshape(3, 3) @ arm + gt[i, 9:] + rng.normal(scale=0.02, size=3), sigma=0.02,
                                lever_arm=arm) for i in range(0, len(gt), 4)]

    def rmse(x):
        return float(np.sqrt(((x[:, 9:] - gt[:, 9:]) ** 2).sum(1).mean()))

    free, _, _ = _prob(pkg, d).refine(x0, max_iter=20)
    p = _prob(pkg, d)
    p.set_priors(fixes)
    x, _, rc = p.refine(x0, max_iter=20)
    assert rc == 0
    assert rmse(free) > 0.5 and rmse(x) < 0.05 and rmse(x) < 0.1 * rmse(free)


def test_refine_is_deterministic_and_ranks_agree(pkg, oracle_mod):
    d = make_problem(**RANKS)
    priors = _mix(d, seed=2)
    a = _prob(pkg, d, priors).refine(d["poses_init"])
    b = _prob(pkg, d, priors).refine(d["poses_init"])
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    orc = po.PriorOracle(oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]), priors)
    xr, tr = orc.damping_iter(d["poses_init"])
    _compare(a[1], tr, a[0], xr)
    N, off, idx, clu = d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]
    V = len(off) - 1
    for world in (2, 4):
        ht = HostTransport(world)

        def rank_main(r):
            lo, hi = pkg.shard_range(V, r, world)
            q = pkg.BalmProblem(N, off[lo:hi + 1], idx[off[lo]:off[hi]], clu[off[lo]:off[hi]])
            ht.attach(q, r)
            q.set_priors([_c(pkg, s) for s in priors])
            H, g, c = q.eval(d["poses_init"])
            x, trace, rc = q.refine(d["poses_init"])
            q.close()
            return dict(H=H, g=g, c=c, x=x, trace=trace, rc=rc)

        out = ht.run(rank_main)
        for o in out[1:]:
            assert np.array_equal(o["H"], out[0]["H"]) and np.array_equal(o["g"], out[0]["g"]) and o["c"] == out[0]["c"]
            assert o["x"].tobytes() == out[0]["x"].tobytes() and o["trace"] == out[0]["trace"]
        assert out[0]["rc"] == 0
        _compare(out[0]["trace"], tr, out[0]["x"], xr)
        assert np.abs(out[0]["x"] - a[0]).max() <= 1e-9


def test_ranks_with_different_priors_are_refused(pkg):
    d = make_problem(n_poses=40, n_voxels=3000, band=10, seed=2)
    N, off, idx, clu = d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]
    V = len(off) - 1
    x = d["poses_gt"].reshape(-1, 12)
    ht = HostTransport(2)

    def rank_main(r):
        lo, hi = pkg.shard_range(V, r, 2)
        q = pkg.BalmProblem(N, off[lo:hi + 1], idx[off[lo]:off[hi]], clu[off[lo]:off[hi]])
        ht.attach(q, r)
        q.set_priors([pkg.Prior.pose(3 + r, x[3 + r], sigma_rot=0.01, sigma_pos=0.1)])
        try:
            q.refine(d["poses_init"])
            return 0
        except pkg._lib.LvbaError as e:
            return e.code
        finally:
            q.close()

    assert ht.run(rank_main) == [pkg._lib.ERR_ARG] * 2


def test_no_priors_changes_no_byte(pkg):
    d = make_problem(**BAND)
    x0 = d["poses_init"]
    ref = _prob(pkg, d)
    cleared = _prob(pkg, d, [])
    replaced = _prob(pkg, d, _mix(d))
    replaced.set_priors([])
    outs = []
    for p in (ref, cleared, replaced):
        H, g, c = p.eval(x0)
        x, trace, rc = p.refine(x0)
        e, ce = p.prior_residuals(x0)
        outs.append((H.tobytes(), g.tobytes(), c, x.tobytes(), trace, p.info()["band_blocks"], p.ordering().tobytes()))
        assert e.shape == (0, 6) and ce == 0.0
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_replacing_priors_after_the_layout(pkg, oracle_mod):
    """After the first evaluation priors may be replaced when their pairs are blocks of the store; blocks that only the old priors
    filled read as zero again."""
    d = make_problem(**CHAIN)
    N = d["n_poses"]
    x = d["poses_gt"].reshape(-1, 12)
    loop = po.make_prior("relative", 0, _rel_gt(x, 0, N - 1), 50.0 * np.eye(6), j=N - 1)
    p = _prob(pkg, d, [loop], band_frac=0.0)          # dense store: every pair is a block
    H1, _, _ = p.eval(d["poses_init"])
    assert np.abs(H1[6 * (N - 1):, :6]).max() > 0
    other = po.make_prior("relative", 3, _rel_gt(x, 3, N - 5), 50.0 * np.eye(6), j=N - 5)
    p.set_priors([_c(pkg, other)])
    H2, g2, c2 = p.eval(d["poses_init"])
    assert not H2[6 * (N - 1):, :6].any() and np.abs(H2[6 * (N - 5):6 * (N - 4), 18:24]).max() > 0
    orc = po.PriorOracle(oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"]), [other])
    Hc, gc, cc = orc.eval_dense(d["poses_init"])
    assert rel(H2, Hc) <= 1e-9 and rel(g2, gc) <= 1e-9


def test_refusals_leave_the_handle_working(pkg, monkeypatch):
    L = pkg._lib
    monkeypatch.setenv("LVBA_SOLVER", "nond")
    d = make_problem(**CHAIN)                         # a narrow band store
    N = d["n_poses"]
    x = d["poses_gt"].reshape(-1, 12)
    p = _prob(pkg, d)
    good = pkg.Prior.pose(2, x[2], sigma_rot=0.01, sigma_pos=0.1)
    p.set_priors([good])
    c_good = p.cost(d["poses_init"])

    def bad(**kw):
        q = pkg.Prior.relative(1, 2, np.eye(4), sigma_rot=0.01, sigma_pos=0.1)
        for k, v in kw.items():
            if k in ("meas", "offset_i", "offset_j", "sqrt_info"):
                getattr(q, k)[:] = list(v)
            else:
                setattr(q, k, v)
        return q

    skew = np.r_[1.01 * np.eye(3).reshape(9), 0, 0, 0]
    cases = [bad(kind=7), bad(i=-1), bad(i=N), bad(j=N), bad(j=1), bad(meas=np.r_[np.eye(3).reshape(9), np.nan, 0, 0]),
             bad(sqrt_info=np.r_[np.inf, np.zeros(35)]), bad(meas=skew), bad(offset_i=skew), bad(offset_j=skew),
             bad(meas=np.r_[np.diag([1.0, 1.0, -1.0]).reshape(9), 0, 0, 0])]
    for q in cases:
        with pytest.raises(L.LvbaError) as e:
            p.set_priors([good, q])
        assert e.value.code == L.ERR_ARG
        assert p.cost(d["poses_init"]) == c_good
    # a pair that is no block of the laid-out band store
    perm = p.ordering()
    assert p.info()["band_blocks"] < N - 1
    far = (int(perm[0]), int(perm[-1]))
    with pytest.raises(L.LvbaError) as e:
        p.set_priors([good, pkg.Prior.relative(*far, np.eye(4), sigma_rot=0.01, sigma_pos=0.1)])
    assert e.value.code == L.ERR_STATE and p.cost(d["poses_init"]) == c_good
    # inside an LM loop
    p.lm_begin(d["poses_init"])
    with pytest.raises(L.LvbaError) as e:
        p.set_priors([])
    assert e.value.code == L.ERR_STATE
    p.lm_step()
    p.lm_end()
    assert p.cost(d["poses_init"]) == c_good
    # grouped handles, in either order
    g1 = _prob(pkg, d)
    g1.set_groups([0, N], [0, len(d["voxel_off"]) - 1])
    with pytest.raises(L.LvbaError) as e:
        g1.set_priors([good])
    assert e.value.code == L.ERR_STATE
    g2 = _prob(pkg, d)
    g2.set_priors([good])
    with pytest.raises(L.LvbaError) as e:
        g2.set_groups([0, N], [0, len(d["voxel_off"]) - 1])
    assert e.value.code == L.ERR_STATE
    assert g2.cost(d["poses_init"]) == c_good
