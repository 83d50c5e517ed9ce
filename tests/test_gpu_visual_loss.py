"""GPU tests of the visual stage's robust losses (lvba_visual_set_loss, lvba_visual_residual_sq) against the reference model
tests/robust_visual_oracle.py (Ceres 2.1's loss functions and Corrector on top of oracle/visual_oracle.py's restated
trust-region loop).  The problems are the synthetic ones of tests/test_gpu_visual.py with a share of the observations
displaced by 20-100 px, so that a fifth or more of the reprojection blocks sit beyond the loss scale."""
import numpy as np
import pytest

from conftest import HostTransport, rel

import robust_visual_oracle as rvo

pytestmark = pytest.mark.gpu

CASES = [dict(n_cams=8, n_tracks=60, seed=3), dict(n_cams=20, n_tracks=300, seed=4, track_len=5),
         dict(n_cams=6, n_tracks=40, seed=5, invalid_frac=0.3)]
REF_LOSSES = (("huber", 1.0), ("huber", 0.1))      # src/lvba_system.cpp:1585-1586


def _mk(pkg, synth, case, frac=0.15, seed=1):
    from oracle import visual_oracle as vo
    d, mask = rvo.add_outliers(synth.make_visual_problem(**case), frac, seed=seed)
    prob = pkg.VisualProblem(d["q"].shape[0], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    p = vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    return d, prob, p


def _equal_runs(a, b):
    (ca, Sa, ra, ta, xa), (cb, Sb, rb, tb, xb) = a, b
    assert ca == cb and np.array_equal(Sa, Sb) and np.array_equal(ra, rb)
    assert ta == tb
    for u, v in zip(xa, xb):
        assert np.array_equal(u, v)


def _run_all(prob, d):
    c = prob.cost(d["q"], d["t"], d["X"])
    S, rhs, _ = prob.linearize(d["q"], d["t"], d["X"], radius=3.0)
    (q, t, X), tr, term, rc = prob.refine(d["q"], d["t"], d["X"])
    return c, S, rhs, (tr, term, rc), (q, t, X)


def test_default_is_unchanged(pkg, synth):
    """set_loss(None, None), and Huber set then reset to trivial, run exactly what a fresh handle runs: bitwise equal cost,
    reduced system and refinement."""
    d, fresh, _ = _mk(pkg, synth, CASES[0])
    ref = _run_all(fresh, d)
    a = pkg.VisualProblem(8, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    a.set_loss(None, None)
    _equal_runs(_run_all(a, d), ref)
    b = pkg.VisualProblem(8, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    b.set_loss(*REF_LOSSES)
    assert b.cost(d["q"], d["t"], d["X"]) < ref[0]
    b.set_loss(("trivial", 1.0), None)
    _equal_runs(_run_all(b, d), ref)
    for h in (fresh, a, b):
        h.close()


@pytest.mark.parametrize("case", CASES)
def test_cost_and_residual_sq_match_oracle(pkg, synth, case):
    d, prob, p = _mk(pkg, synth, case)
    base = rvo.RobustVisualOracle(p)
    q, t, X = base.state()
    r, _ = rvo.VisualOracle.residuals_and_jacobian(base, q, t, X, want_jac=False)
    s = base.block_sq(r)
    fam = base.block_family
    assert (s[fam == 0] > 1.0).mean() >= 0.2
    # residual_sq: caller order, NaN exactly on the inactive landmarks and their observations
    obs_sq, pl_sq = prob.residual_sq(q, t, X)
    obs_ref, pl_ref = np.full(len(d["obs_uv"]), np.nan), np.full(len(d["valid"]), np.nan)
    for b, (kind, _li, ti, o) in enumerate(base.rows):
        if kind == "r":
            obs_ref[o] = s[b]
        else:
            pl_ref[ti] = s[b]
    assert np.array_equal(np.isnan(obs_sq), np.isnan(obs_ref)) and np.array_equal(np.isnan(pl_sq), np.isnan(pl_ref))
    assert np.array_equal(np.isnan(pl_sq), d["valid"] == 0)
    fin = ~np.isnan(obs_ref)
    assert rel(obs_sq[fin], obs_ref[fin]) <= 1e-12 and rel(pl_sq[~np.isnan(pl_ref)], pl_ref[~np.isnan(pl_ref)]) <= 1e-12
    configs = [((k, 1.0), None) for k in rvo.KINDS if k != "trivial"] + [(None, ("huber", 0.1)), (("huber", 1.0), ("cauchy", 0.1))]
    for lr, lp in configs:
        c_ref = 0.5 * rvo.RobustVisualOracle(p, lr, lp).block_rho(s)[:, 0].sum()
        prob.set_loss(lr, lp)
        c = prob.cost(q, t, X)
        assert abs(c - c_ref) <= 1e-10 * c_ref, (lr, lp, c, c_ref)
    prob.close()


@pytest.mark.parametrize("case", CASES)
def test_reduced_camera_system_matches_oracle(pkg, synth, case):
    """S and rhs of the corrected Jacobian (Jacobi scaling from J~ as well) against the oracle's dense Schur complement."""
    d, prob, p = _mk(pkg, synth, case)
    base = rvo.VisualOracle(p)
    q, t, X = base.state()
    r, J = base.residuals_and_jacobian(q, t, X)
    for lr in (("huber", 1.0), ("cauchy", 1.0), ("tukey", 3.0)):
        orc = rvo.RobustVisualOracle(p, lr, ("huber", 0.1))
        corr = orc.correct(r, J)
        prob.set_loss(lr, ("huber", 0.1))
        for radius in (1e4, 3.0):
            S_ref, rhs_ref, c_ref = orc.reduced_system(*corr, radius)
            S, rhs, c = prob.linearize(q, t, X, radius)
            assert abs(c - c_ref) <= 1e-10 * c_ref
            assert rel(S[6:, 6:], S_ref) <= 1e-9, (lr, radius, rel(S[6:, 6:], S_ref))
            assert rel(rhs[6:], rhs_ref) <= 1e-9
            assert np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0
            assert np.array_equal(S, S.T)
    prob.close()


TRACE_CASES = [(dict(n_cams=8, n_tracks=60, seed=3), 1e-7, (1e-8, 1e-7, 1e-7)),
               # a farther start: the oracle's Huber run rejects its second step (46 rows), the Cauchy run has 13 rows
               (dict(n_cams=8, n_tracks=60, seed=3, rot_sigma_deg=0.8, trans_sigma=0.15, point_sigma=0.3), 1e-6, (1e-7, 1e-6, 1e-6))]


@pytest.mark.parametrize("case,cost_tol,state_tol", TRACE_CASES)
def test_refine_trace_matches_oracle(pkg, synth, case, cost_tol, state_tol):
    rejected = 0
    for lr, lp in (REF_LOSSES, (("cauchy", 2.0), None)):
        d, prob, p = _mk(pkg, synth, case)
        prob.set_loss(lr, lp)
        (q, t, X), trace, term, rc = prob.refine(d["q"], d["t"], d["X"])
        (qr, tr, Xr), trace_ref, term_ref = rvo.RobustVisualOracle(p, lr, lp).solve()
        assert rc == 0 and term == term_ref and len(trace) == len(trace_ref), (lr, term, term_ref, len(trace), len(trace_ref))
        for a, b in zip(trace, trace_ref):
            assert a["accepted"] == b["accepted"]
            assert abs(a["cost"] - b["cost"]) <= cost_tol * abs(b["cost"])
            assert abs(a["radius"] - b["radius"]) <= 1e-6 * b["radius"]
        assert np.abs(q - qr).max() <= state_tol[0] and np.abs(t - tr).max() <= state_tol[1] and np.abs(X - Xr).max() <= state_tol[2]
        assert trace[-1]["cost"] < trace[0]["cost"]
        rejected += sum(1 for b in trace_ref[1:-1] if not b["accepted"])         # (the last row: a tolerance test)
        prob.close()
    if case.get("rot_sigma_deg"):
        assert rejected >= 1                                                 # rows after a rejection were compared too


def _cam_err(d, q, t):
    dq = np.abs(np.sum(q * d["q_gt"], 1)).clip(max=1.0)
    return float(np.sqrt(np.mean(np.sum((t - d["t_gt"]) ** 2, 1)))), float(np.sqrt(np.mean((2.0 * np.arccos(dq)) ** 2)))


def test_huber_is_robust_to_gross_outliers(pkg, synth):
    """20 cameras x 300 landmarks, 10 % of the observations displaced by 20-100 px: the reference's Huber losses bring the
    cameras closer to the ground truth than the plain least squares.  The CPU oracle (tests/robust_visual_oracle.py) on this
    seed and outlier seed gives RMS camera errors, translation / rotation: start 0.0286 m / 0.00164 rad, trivial 0.352 m /
    0.0189 rad, Huber 0.0312 m / 0.00190 rad -- Huber / trivial = 0.089 / 0.101.  The bar, 0.3, leaves a factor 3 of margin."""
    d, prob, _ = _mk(pkg, synth, dict(n_cams=20, n_tracks=300, seed=4, track_len=5), frac=0.10, seed=7)
    (q0, t0, _), _, _, rc0 = prob.refine(d["q"], d["t"], d["X"])
    prob.set_loss(*REF_LOSSES)
    (q1, t1, _), tr1, _, rc1 = prob.refine(d["q"], d["t"], d["X"])
    assert rc0 == rc1 == 0
    et0, er0 = _cam_err(d, q0, t0)
    et1, er1 = _cam_err(d, q1, t1)
    assert et1 < 0.3 * et0 and er1 < 0.3 * er0, (et0, et1, er0, er1)
    prob.close()


def _shard_run(pkg, d, world, losses):
    n_cams, n_tracks = d["q"].shape[0], len(d["obs_off"]) - 1
    off, cam, uv = d["obs_off"], d["obs_cam"], d["obs_uv"]
    ht = HostTransport(world)

    def rank_main(r):
        a, b = pkg.shard_range(n_tracks, r, world)
        vp = pkg.VisualProblem(n_cams, off[a:b + 1], cam[off[a]:off[b]], uv[off[a]:off[b]], d["plane"][a:b], d["valid"][a:b], d["intr"])
        ht.attach(vp, r)
        vp.set_loss(*losses[r])
        try:
            c = vp.cost(d["q"], d["t"], d["X"][a:b])
            S, rhs, _ = vp.linearize(d["q"], d["t"], d["X"][a:b], radius=3.0)
            (q, t, X), tr, term, rc = vp.refine(d["q"], d["t"], d["X"][a:b])
            return dict(c=c, S=S, rhs=rhs, q=q, t=t, X=X, tr=tr, term=term, rc=rc)
        except pkg._lib.LvbaError as e:
            return dict(err=e.code)
        finally:
            vp.close()

    return ht.run(rank_main, timeout=120)


@pytest.mark.parametrize("world,n_cams,n_tracks", [(2, 40, 1500), (3, 12, 300)])
def test_sharded_huber_agrees_with_single_rank(pkg, synth, world, n_cams, n_tracks):
    d, mask = rvo.add_outliers(synth.make_visual_problem(n_cams, n_tracks, seed=11), 0.15, seed=2)
    one = pkg.VisualProblem(n_cams, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    one.set_loss(*REF_LOSSES)
    c1 = one.cost(d["q"], d["t"], d["X"])
    S1, rhs1, _ = one.linearize(d["q"], d["t"], d["X"], radius=3.0)
    (q1, t1, X1), tr1, term1, rc1 = one.refine(d["q"], d["t"], d["X"])
    one.close()
    out = _shard_run(pkg, d, world, [REF_LOSSES] * world)
    r0 = out[0]
    for o in out[1:]:
        assert o["c"] == r0["c"] and np.array_equal(o["S"], r0["S"]) and np.array_equal(o["rhs"], r0["rhs"])
        assert np.array_equal(o["q"], r0["q"]) and np.array_equal(o["t"], r0["t"]) and o["term"] == r0["term"]
        assert [row["cost"] for row in o["tr"]] == [row["cost"] for row in r0["tr"]]
    assert abs(r0["c"] - c1) <= 1e-12 * c1
    assert rel(r0["S"], S1) <= 1e-11 and rel(r0["rhs"], rhs1) <= 1e-11
    assert r0["rc"] == rc1 == 0 and r0["term"] == term1 and len(r0["tr"]) == len(tr1)
    for a_, b_ in zip(r0["tr"], tr1):
        assert a_["accepted"] == b_["accepted"] and abs(a_["cost"] - b_["cost"]) <= 1e-8 * b_["cost"]
    assert np.abs(r0["q"] - q1).max() <= 1e-8 and np.abs(r0["t"] - t1).max() <= 1e-8
    assert np.abs(np.concatenate([o["X"] for o in out]) - X1).max() <= 1e-7


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_with_different_losses_all_fail(pkg, synth, world):
    """One rank with another loss scale: every rank gets LVBA_ERR_ARG from its first collective call, none waits."""
    d = synth.make_visual_problem(12, 300, seed=11)
    losses = [REF_LOSSES] * world
    losses[world - 1] = (("huber", 2.0), ("huber", 0.1))
    out = _shard_run(pkg, d, world, losses)
    assert [o.get("err") for o in out] == [pkg._lib.ERR_ARG] * world
    losses[world - 1] = (None, ("huber", 0.1))                 # another kind
    out = _shard_run(pkg, d, world, losses)
    assert [o.get("err") for o in out] == [pkg._lib.ERR_ARG] * world


def test_robust_linearization_at_c3_scale(pkg, synth):
    """The ROBUST kernels at the visual stage's C3 size (2 000 cameras x 125 000 landmarks): Huber with a = 1e6 keeps every block
    an inlier (rho' = 1), so its linearisation must equal the trivial one."""
    import torch
    M, T = 2000, 125_000
    d = synth.make_visual_problem(M, T, device="cuda")
    torch.cuda.synchronize()
    args = (d["q"], d["t"], d["X"])
    prob = pkg.VisualProblem(M, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    S0, rhs0, c0 = prob.linearize(*args, 1e4)
    prob.set_loss(("huber", 1e6), ("huber", 1e6))
    S1, rhs1, c1 = prob.linearize(*args, 1e4)
    assert abs(c1 - c0) <= 1e-13 * c0
    assert rel(S1, S0) <= 1e-13 and rel(rhs1, rhs0) <= 1e-13
    del S0, S1
    prob.close()


def test_argument_checks(pkg, synth):
    import ctypes as C
    L = pkg._lib
    lib = L.load()
    d, prob, _ = _mk(pkg, synth, CASES[0])
    prob.set_loss(*REF_LOSSES)
    c = prob.cost(d["q"], d["t"], d["X"])
    bad = [L.Loss(9, 0, 1.0), L.Loss(-1, 0, 1.0), L.Loss(1, 0, 0.0), L.Loss(3, 0, -1.0), L.Loss(5, 0, float("nan")),
           L.Loss(2, 0, float("inf"))]
    for b in bad:
        assert lib.lvba_visual_set_loss(prob._h, C.byref(b), None) == L.ERR_ARG
        assert lib.lvba_visual_set_loss(prob._h, None, C.byref(b)) == L.ERR_ARG
        assert prob.cost(d["q"], d["t"], d["X"]) == c                   # the handle kept its losses
    for kw in (dict(reproj=("huber", 0.0)), dict(plane=("cauchy", -1.0)), dict(reproj=("tukey", float("nan"))), dict(reproj=(7, 1.0))):
        with pytest.raises(L.LvbaError):
            prob.set_loss(**kw)
    assert prob.cost(d["q"], d["t"], d["X"]) == c
    with pytest.raises(ValueError):
        prob.set_loss(("welsch", 1.0))
    assert lib.lvba_visual_set_loss(None, None, None) == L.ERR_ARG
    q, t, X = prob._state(d["q"], d["t"], d["X"])
    buf = np.empty(len(d["obs_uv"]) + len(d["valid"]))
    assert lib.lvba_visual_residual_sq(None, q, t, X, buf.ctypes.data, buf.ctypes.data) == L.ERR_ARG
    assert lib.lvba_visual_residual_sq(prob._h, q, t, X, None, buf.ctypes.data) == L.ERR_ARG
    assert lib.lvba_visual_residual_sq(prob._h, q, t, X, buf.ctypes.data, None) == L.ERR_ARG
    prob.close()
