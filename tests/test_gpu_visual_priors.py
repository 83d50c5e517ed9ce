"""GPU tests of the visual stage's camera pose priors (lvba_visual_set_priors, lvba_visual_prior_residuals) against the reference
model tests/visual_prior_oracle.py (the three prior residuals on T_world<-cam in torch, appended as residual blocks to
tests/robust_visual_oracle.py's restated trust-region loop).  The problems are the synthetic ones of tests/test_gpu_visual_loss.py;
the priors (visual_prior_cases.mixed_priors) mix all three kinds, offsets and lever arms, and include one on camera 0, one
RELATIVE pair that shares no landmark and RELATIVE pairs with camera 0."""
import ctypes as C

import numpy as np
import pytest

from conftest import HostTransport, rel

import robust_visual_oracle as rvo
import visual_prior_cases as vc
import visual_prior_oracle as vpo

pytestmark = pytest.mark.gpu

SMALL = dict(n_cams=8, n_tracks=60, seed=3)
LOSSES = ((None, None), (("huber", 1.0), ("huber", 0.1)))
# the cases and per-case bars of tests/test_gpu_visual_loss.py's TRACE_CASES
TRACE_CASES = [(dict(n_cams=8, n_tracks=60, seed=3), 1e-7, (1e-8, 1e-7, 1e-7)),
               (dict(n_cams=8, n_tracks=60, seed=3, rot_sigma_deg=0.8, trans_sigma=0.15, point_sigma=0.3), 1e-6, (1e-7, 1e-6, 1e-6))]


def _mk(pkg, synth, case, outliers=True):
    from oracle import visual_oracle as vo
    d = synth.make_visual_problem(**case)
    if outliers:
        d, _ = rvo.add_outliers(d, 0.15, seed=1)
    prob = pkg.VisualProblem(d["q"].shape[0], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    p = vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    return d, prob, p


def _handle(pkg, d):
    return pkg.VisualProblem(d["q"].shape[0], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])


def _run_all(prob, d):
    c = prob.cost(d["q"], d["t"], d["X"])
    S, rhs, _ = prob.linearize(d["q"], d["t"], d["X"], radius=3.0)
    (q, t, X), tr, term, rc = prob.refine(d["q"], d["t"], d["X"])
    return c, S, rhs, (tr, term, rc), (q, t, X)


def _equal_runs(a, b):
    (ca, Sa, ra, ta, xa), (cb, Sb, rb, tb, xb) = a, b
    assert ca == cb and np.array_equal(Sa, Sb) and np.array_equal(ra, rb)
    assert ta == tb
    for u, v in zip(xa, xb):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("losses", LOSSES)
def test_residuals_cost_and_reduced_system_match_oracle(pkg, synth, losses):
    """prior_residuals 1e-12, cost 1e-10, S and rhs 1e-9 relative at two radii (the bars tests/test_gpu_visual_loss.py holds the
    same quantities to), on 8 cameras (dense store) and 20 cameras, with trivial and with both losses non-trivial."""
    for case in (SMALL, dict(n_cams=20, n_tracks=300, seed=4, track_len=5)):
        d, prob, p = _mk(pkg, synth, case)
        priors = vc.mixed_priors(synth, d)
        orc = vpo.VisualPriorOracle(p, priors, *losses)
        q, t, X = orc.state()
        prob.set_loss(*losses)
        prob.set_priors(priors)
        e, c = prob.prior_residuals(q, t)
        e_ref, c_ref = orc.prior_residuals(q, t)
        print("prior residuals", rel(e, e_ref), "prior cost", abs(c - c_ref) / c_ref)
        assert rel(e, e_ref) <= 1e-12 and abs(c - c_ref) <= 1e-12 * c_ref
        assert any(int(pr.kind) == 1 for pr in priors) and all(not e[k, 3:].any() for k, pr in enumerate(priors) if int(pr.kind) == 1)
        lin = orc.residuals_and_jacobian(q, t, X)
        cost_ref = orc._cost(lin[0], lin[3])
        cost = prob.cost(q, t, X)
        print("cost", abs(cost - cost_ref) / cost_ref)
        assert abs(cost - cost_ref) <= 1e-10 * cost_ref
        for radius in (1e4, 3.0):
            S_ref, rhs_ref, c_lin = orc.reduced_system(*lin, radius)
            S, rhs, cl = prob.linearize(q, t, X, radius)
            print(case["n_cams"], losses[0], radius, "S", rel(S[6:, 6:], S_ref), "rhs", rel(rhs[6:], rhs_ref))
            assert abs(cl - c_lin) <= 1e-10 * c_lin
            assert rel(S[6:, 6:], S_ref) <= 1e-9 and rel(rhs[6:], rhs_ref) <= 1e-9
            assert np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0
            assert np.array_equal(S, S.T)
        prob.close()


def test_linearization_with_a_few_hundred_cameras(pkg, synth):
    """180 cameras (RCM order, banded store): a RELATIVE pair far outside the co-visibility band and one with camera 0, set before
    the first call, widen the band; cost, S and rhs against the oracle at two radii."""
    M = 180
    d, prob, p = _mk(pkg, synth, dict(n_cams=M, n_tracks=900, seed=12), outliers=False)
    bb0 = prob.info()["band_blocks"]
    prob.close()
    I12 = np.r_[np.eye(3).reshape(9), 0.3, -0.2, 0.1]
    priors = vc.mixed_priors(synth, d) + [vc.make_prior(2, 10, 150, I12, np.eye(6) * 2.0), vc.make_prior(2, 0, 100, I12, np.eye(6))]
    prob = _handle(pkg, d)
    prob.set_priors(priors)
    assert prob.info()["band_blocks"] > bb0
    orc = vpo.VisualPriorOracle(p, priors)
    q, t, X = orc.state()
    lin = orc.residuals_and_jacobian(q, t, X)
    for radius in (1e4, 3.0):
        S_ref, rhs_ref, c_ref = orc.reduced_system(*lin, radius)
        S, rhs, c = prob.linearize(q, t, X, radius)
        print(radius, "cost", abs(c - c_ref) / c_ref, "S", rel(S[6:, 6:], S_ref), "rhs", rel(rhs[6:], rhs_ref))
        assert abs(c - c_ref) <= 1e-10 * c_ref
        assert rel(S[6:, 6:], S_ref) <= 1e-9 and rel(rhs[6:], rhs_ref) <= 1e-9
        assert np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0 and np.array_equal(S, S.T)
        assert np.abs(S[60:66, 900:906]).max() > 0.0                  # the block of the far pair (10, 150)
    prob.close()


@pytest.mark.parametrize("case,cost_tol,state_tol", TRACE_CASES)
def test_refine_trace_matches_oracle(pkg, synth, case, cost_tol, state_tol):
    # the losses tests/test_gpu_visual_loss.py runs these cases with, on its outlier data; the trivial loss on the clean problem
    # (plain least squares on 20-100 px outliers is no case either file holds to these bars: measured here with these priors,
    # costs agree to 3e-9 over 19 rows, then a rejected step's candidate cost differs by 9.4e-7; on the farther start all 51 rows
    # agree to 1.2e-12 and q, t to 3e-11 while one landmark differs by 1.1e-3)
    for losses, outliers in ((LOSSES[1], True), ((("cauchy", 2.0), None), True), (LOSSES[0], False)):
        d, prob, p = _mk(pkg, synth, case, outliers)
        priors = vc.mixed_priors(synth, d)
        prob.set_loss(*losses)
        prob.set_priors(priors)
        (q, t, X), trace, term, rc = prob.refine(d["q"], d["t"], d["X"])
        (qr, tr, Xr), trace_ref, term_ref = vpo.VisualPriorOracle(p, priors, *losses).solve()
        # Compare up to the first row where the oracle's own |cost_change| is at rounding level: two fp64 sums of the n_rows squared
        # residuals in different orders differ by up to n_rows eps cost, rho = cost_change / model_change inherits that over
        # |cost_change|, and the radius update 1 - (2 rho - 1)^3 passes it on with a factor <= 6 -- below
        # 6 n_rows eps cost / 1e-6 the radius cannot be held to its 1e-6 bar by any two correct implementations.
        n_rows = 2 * len(d["obs_uv"]) + len(d["valid"]) + 6 * len(priors)
        level = 6.0 * n_rows * np.finfo(np.float64).eps / 1e-6
        n = len(trace_ref)
        for k, b in enumerate(trace_ref[1:], 1):
            if abs(b["cost_change"]) <= level * abs(b["cost"]):
                n = k
                break
        print(losses[0], term, term_ref, len(trace), len(trace_ref), "rows compared", n)
        assert rc == 0 and len(trace) >= n
        if n == len(trace_ref):
            assert term == term_ref and len(trace) == len(trace_ref)
        for a, b in zip(trace[:n], trace_ref[:n]):
            print(a["iter"], a["accepted"], b["accepted"], abs(a["cost"] - b["cost"]) / abs(b["cost"]), abs(a["radius"] - b["radius"]) / b["radius"],
                  "oracle cost_change / cost", b["cost_change"] / b["cost"])
            assert a["accepted"] == b["accepted"]
            assert abs(a["cost"] - b["cost"]) <= cost_tol * abs(b["cost"])
            assert abs(a["radius"] - b["radius"]) <= 1e-6 * b["radius"]
        print("state", np.abs(q - qr).max(), np.abs(t - tr).max(), np.abs(X - Xr).max())
        assert np.abs(q - qr).max() <= state_tol[0] and np.abs(t - tr).max() <= state_tol[1] and np.abs(X - Xr).max() <= state_tol[2]
        assert trace[-1]["cost"] < trace[0]["cost"]
        prob.close()


def test_no_priors_is_bitwise_today_and_runs_repeat(pkg, synth):
    d, fresh, _ = _mk(pkg, synth, SMALL)
    ref = _run_all(fresh, d)
    a = _handle(pkg, d)
    a.set_priors([])
    _equal_runs(_run_all(a, d), ref)
    b = _handle(pkg, d)
    priors = vc.mixed_priors(synth, d)
    b.set_priors(priors)
    with_p = _run_all(b, d)
    assert with_p[0] > ref[0]
    b.set_priors(None)                                                # cleared after use: prior-only blocks are zero again
    _equal_runs(_run_all(b, d), ref)
    c = _handle(pkg, d)
    c.set_priors(priors)
    c.set_priors([])                                                  # cleared before the first call
    _equal_runs(_run_all(c, d), ref)
    e = _handle(pkg, d)
    e.set_priors(priors)
    _equal_runs(_run_all(e, d), with_p)                                # two runs with priors: byte-identical
    _equal_runs(_run_all(e, d), with_p)
    for h in (fresh, a, b, c, e):
        h.close()
    # a banded store as well (prior-only blocks are written, then zeroed when the priors go)
    d = synth.make_visual_problem(300, 3000, seed=12)
    f = _handle(pkg, d)
    ref = f.linearize(d["q"], d["t"], d["X"], 3.0)
    g = _handle(pkg, d)
    g.set_priors(vc.mixed_priors(synth, d))
    g.linearize(d["q"], d["t"], d["X"], 3.0)
    g.set_priors([])
    got = g.linearize(d["q"], d["t"], d["X"], 3.0)
    assert got[2] == ref[2] and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    f.close()
    g.close()


def test_error_paths(pkg, synth):
    L = pkg._lib
    lib = L.load()
    d = synth.make_visual_problem(300, 3000, seed=12)
    M = 300
    prob = _handle(pkg, d)
    good = vc.mixed_priors(synth, d)
    prob.set_priors(good)
    ref = prob.linearize(d["q"], d["t"], d["X"], 3.0)
    e_ref = prob.prior_residuals(d["q"], d["t"])

    def same():
        got = prob.linearize(d["q"], d["t"], d["X"], 3.0)
        e = prob.prior_residuals(d["q"], d["t"])
        return got[2] == ref[2] and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(e[0], e_ref[0])

    I12 = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    bad_rot = I12.copy()
    bad_rot[0] = 1.001
    nan_m = I12.copy()
    nan_m[10] = np.nan
    Lnan = np.eye(6)
    Lnan[2, 1] = np.inf
    bad = [vc.make_prior(7, 1, 0, I12, np.eye(6)), vc.make_prior(-1, 1, 0, I12, np.eye(6)), vc.make_prior(0, M, 0, I12, np.eye(6)),
           vc.make_prior(0, -1, 0, I12, np.eye(6)), vc.make_prior(2, 1, M, I12, np.eye(6)), vc.make_prior(2, 5, 5, I12, np.eye(6)),
           vc.make_prior(0, 1, 0, nan_m, np.eye(6)), vc.make_prior(0, 1, 0, I12, Lnan), vc.make_prior(0, 1, 0, bad_rot, np.eye(6)),
           vc.make_prior(0, 1, 0, I12, np.eye(6), oi=bad_rot), vc.make_prior(2, 1, 2, I12, np.eye(6), oj=bad_rot)]
    for b in bad:
        arr = (L.Prior * 2)(good[0], b)
        assert lib.lvba_visual_set_priors(prob._h, 2, C.cast(arr, C.c_void_p)) == L.ERR_ARG
        assert same()
    assert lib.lvba_visual_set_priors(prob._h, -1, None) == L.ERR_ARG and lib.lvba_visual_set_priors(prob._h, 1, None) == L.ERR_ARG
    assert lib.lvba_visual_set_priors(prob._h, (1 << 22) + 1, C.cast((L.Prior * 1)(good[0]), C.c_void_p)) == L.ERR_ARG
    assert lib.lvba_visual_set_priors(None, 0, None) == L.ERR_ARG
    assert lib.lvba_visual_prior_residuals(None, d["q"].reshape(-1), d["t"].reshape(-1), None, None) == L.ERR_ARG
    assert same()
    # a new pair after the first linearisation: far outside the band
    far = vc.make_prior(2, 10, 200, I12, np.eye(6))
    assert prob.info()["band_blocks"] < 150
    arr = (L.Prior * 1)(far)
    assert lib.lvba_visual_set_priors(prob._h, 1, C.cast(arr, C.c_void_p)) == L.ERR_STATE
    assert same()
    # replacing the priors on pairs the store holds works, and changes the result
    prob.set_priors(good[:-1])
    assert not np.array_equal(prob.linearize(d["q"], d["t"], d["X"], 3.0)[0], ref[0])
    prob.set_priors(good)
    assert same()
    prob.close()


def _shard_run(pkg, d, world, priors_of_rank):
    n_cams, n_tracks = d["q"].shape[0], len(d["obs_off"]) - 1
    off, cam, uv = d["obs_off"], d["obs_cam"], d["obs_uv"]
    ht = HostTransport(world)

    def rank_main(r):
        a, b = pkg.shard_range(n_tracks, r, world)
        vp = pkg.VisualProblem(n_cams, off[a:b + 1], cam[off[a]:off[b]], uv[off[a]:off[b]], d["plane"][a:b], d["valid"][a:b], d["intr"])
        ht.attach(vp, r)
        vp.set_loss(("huber", 1.0), ("huber", 0.1))
        vp.set_priors(priors_of_rank[r])
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


def test_sharded_agrees_with_single_rank(pkg, synth):
    """Two host-thread ranks (tests/host_transport.cpp): rank 0 alone adds the priors; trace and cameras equal the one-rank run
    to the bars of tests/test_gpu_visual_loss.py's sharded case."""
    n_cams, n_tracks, world = 40, 1500, 2
    d, _ = rvo.add_outliers(synth.make_visual_problem(n_cams, n_tracks, seed=11), 0.15, seed=2)
    priors = vc.mixed_priors(synth, d)
    one = _handle(pkg, d)
    one.set_loss(("huber", 1.0), ("huber", 0.1))
    one.set_priors(priors)
    c1 = one.cost(d["q"], d["t"], d["X"])
    S1, rhs1, _ = one.linearize(d["q"], d["t"], d["X"], radius=3.0)
    (q1, t1, X1), tr1, term1, rc1 = one.refine(d["q"], d["t"], d["X"])
    one.close()
    out = _shard_run(pkg, d, world, [priors] * world)
    r0 = out[0]
    for o in out[1:]:
        assert o["c"] == r0["c"] and np.array_equal(o["S"], r0["S"]) and np.array_equal(o["rhs"], r0["rhs"])
        assert np.array_equal(o["q"], r0["q"]) and np.array_equal(o["t"], r0["t"]) and o["term"] == r0["term"]
        assert [row["cost"] for row in o["tr"]] == [row["cost"] for row in r0["tr"]]
    print("cost", abs(r0["c"] - c1) / c1, "S", rel(r0["S"], S1), "rhs", rel(r0["rhs"], rhs1))
    assert abs(r0["c"] - c1) <= 1e-12 * c1
    assert rel(r0["S"], S1) <= 1e-11 and rel(r0["rhs"], rhs1) <= 1e-11
    assert r0["rc"] == rc1 == 0 and r0["term"] == term1 and len(r0["tr"]) == len(tr1)
    for a_, b_ in zip(r0["tr"], tr1):
        assert a_["accepted"] == b_["accepted"] and abs(a_["cost"] - b_["cost"]) <= 1e-8 * b_["cost"]
    assert np.abs(r0["q"] - q1).max() <= 1e-8 and np.abs(r0["t"] - t1).max() <= 1e-8
    assert np.abs(np.concatenate([o["X"] for o in out]) - X1).max() <= 1e-7


def test_sharded_ranks_with_different_priors_all_fail(pkg, synth):
    d = synth.make_visual_problem(12, 300, seed=11)
    priors = vc.mixed_priors(synth, d)
    other = list(priors)
    other[2] = vc.make_prior(0, 2, 0, np.r_[np.eye(3).reshape(9), 0.5, 0.0, 0.0], np.eye(6))
    for variant in (other, priors[:-1], []):
        out = _shard_run(pkg, d, 2, [priors, variant])
        assert [o.get("err") for o in out] == [pkg._lib.ERR_ARG] * 2


def test_priors_pull_drifted_cameras_back(pkg, synth):
    """visual_prior_cases.drift_case (8 cameras x 60 landmarks, seed 3, a smooth drift growing to 6 cm / 0.3 deg along the
    trajectory, POSE priors at the true poses from pipeline.lidar_camera_priors, sigma 0.0005 rad / 0.003 m): the refined
    camera-centre RMS error with priors is below DRIFT_BAR = 0.19 of the one without.  The oracle alone
    (tests/test_visual_priors_host.py) gives 0.02013 m without, 0.001903 m with: ratio 0.0945; the bar is twice that."""
    d, _, priors = vc.drift_case(pkg, synth)
    prob = _handle(pkg, d)
    (q0, t0, _), _, _, rc0 = prob.refine(d["q"], d["t"], d["X"])
    prob.set_priors(priors)
    (q1, t1, _), _, _, rc1 = prob.refine(d["q"], d["t"], d["X"])
    prob.close()
    e0, e1 = vc.centre_rms(d, q0, t0), vc.centre_rms(d, q1, t1)
    print("camera-centre RMS without / with priors:", e0, e1, "ratio", e1 / e0)
    assert rc0 == rc1 == 0
    assert e1 < vc.DRIFT_BAR * e0


def test_optimize_camera_poses_takes_priors(pkg, synth):
    d, _, priors = vc.drift_case(pkg, synth)
    args = (d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"][:, :3], d["plane"][:, 3], d["intr"])
    (q0, t0, _), *_ = pkg.optimize_camera_poses(*args)
    (q1, t1, _), *_ = pkg.optimize_camera_poses(*args, priors=priors)
    assert vc.centre_rms(d, q1, t1) < vc.DRIFT_BAR * vc.centre_rms(d, q0, t0)
