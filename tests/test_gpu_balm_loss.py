"""GPU tests of the robust losses of the LiDAR bundle adjustment (lvba_balm_set_loss, lvba_balm_voxel_residuals,
lvba_lidar_ba_robust) against the reference model tests/robust_balm_oracle.py.

Inputs: synthetic problems of the sizes the small parity tests use, a quarter of the voxels with one cluster displaced by
5 a .. 20 a, the scale a derived from the data (a^2 = 4 x the 90th percentile of lambda_min of the untouched problem).  Every test
that uses them first asserts, on the oracle's values, that >= 10 % of the voxels lie above a^2 and >= 75 % at or below it.
Tolerances: DESIGN.md section 2 -- 1e-8 relative on cost, g, H; 1e-7 on per-iteration LM costs and final poses."""
import importlib

import numpy as np
import pytest

import prior_oracle as po
import robust_balm_oracle as rbo
from conftest import HostTransport, make_problem, rel
from oracle import balm_oracle as bo
from test_gpu_balm import _compare_traces

pytestmark = pytest.mark.gpu

SMALL = dict(n_poses=12, n_voxels=150, band=6, seed=7)
MID = dict(n_poses=40, n_voxels=3000, band=10, seed=2)
KINDS = ["huber", "softlone", "cauchy", "arctan", "tukey"]


def _inputs(case):
    d = make_problem(**case)
    dc, touched, a = rbo.contaminated(d)
    rbo.check_input_shares(dc, a)
    return d, dc, touched, a


def _prob(pkg, d, **kw):
    return pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"], **kw)


def _rows(tr):
    """oracle trace rows in the tuple layout _compare_traces reads"""
    return [(r.it, r.residual1, r.residual2, r.u, r.v, r.q, r.q1, r.accepted, r.evaluated) for r in tr]


def test_default_is_unchanged_and_huber_lowers_the_cost(pkg):
    """set_loss(None), and Huber set and reset to trivial, give bitwise the cost, H, g and refinement of a fresh handle."""
    _, dc, _, a = _inputs(MID)
    x0 = dc["poses_init"]
    ref = _prob(pkg, dc)
    c0, (H0, g0, ca0) = ref.cost(x0), ref.eval(x0)
    xr, tr, rc = ref.refine(x0)
    p1 = _prob(pkg, dc)
    p1.set_loss(None)
    p2 = _prob(pkg, dc)
    p2.set_loss(("huber", a))
    ch = p2.cost(x0)
    assert ch < c0
    Hh, gh, _ = p2.eval(x0)
    assert not np.array_equal(Hh, H0) and not np.array_equal(gh, g0)
    p2.set_loss(("trivial", 0.0))
    for p in (p1, p2):
        assert p.cost(x0) == c0
        H, g, ca = p.eval(x0)
        assert np.array_equal(H, H0) and np.array_equal(g, g0) and ca == ca0
        x, t, r = p.refine(x0)
        assert r == rc and np.array_equal(x, xr) and t == tr
        lam, w = p.voxel_residuals(x0)
        assert (w == 1.0).all()
    for p in (ref, p1, p2):
        p.close()


@pytest.mark.parametrize("kind,mult", [(k, 1.0) for k in KINDS] + [("huber", 0.5), ("huber", 2.0)])
def test_cost_gradient_and_hessian_match_the_oracle(pkg, kind, mult):
    _, dc, _, a = _inputs(MID)
    a *= mult
    x0 = dc["poses_init"]
    Ho, go, co_, lam, w = rbo.evaluate(rbo.problem(dc), x0, kind, a)
    p = _prob(pkg, dc)
    p.set_loss((kind, a))
    c = p.cost(x0)
    H, g, ca = p.eval(x0)
    print(f"{kind} a={a:.4f}: cost {abs(c - co_) / co_:.2e} g {rel(g, go):.2e} H {rel(H, Ho):.2e}")
    assert abs(c - co_) <= 1e-8 * co_ and abs(ca * p.n_voxels - co_) <= 1e-8 * co_
    assert rel(g, go) <= 1e-8 and rel(H, Ho) <= 1e-8
    assert np.array_equal(H, H.T)
    p.close()


def test_cost_call_equals_eval_cost_bitwise(pkg):
    """lvba_balm_cost (the cost-only kernel) and lvba_balm_eval (the voxel pass) sum the same rho values in the same order."""
    _, dc, _, a = _inputs(MID)
    for kind in KINDS:
        p = _prob(pkg, dc)
        p.set_loss((kind, a))
        for x in (dc["poses_init"], dc["poses_gt"]):
            assert p.cost(x, is_avg=True) == p.eval(x, want_H=False, want_g=False)[2]
        p.close()


def test_big_voxel_branch(pkg):
    """One voxel with more observers than a workgroup has lanes (merged in tiles, a chunk of its own), displaced like the others'
    outliers so that it is down-weighted: cost, g, H against the oracle, cost call against eval bitwise."""
    rng = np.random.default_rng(7)
    N = 300
    d = make_problem(N, 400, band=12, seed=5)
    off, idx, clu = d["voxel_off"], d["pose_idx"], d["clusters"].reshape(-1, 10)
    poses = np.sort(rng.choice(N, 280, replace=False))
    out = []
    for k, pz in enumerate(poses):
        T = d["poses_gt"][pz]
        R, tr = T[:9].reshape(3, 3), T[9:]
        pw = np.column_stack([rng.uniform(-0.4, 0.4, (20, 2)) + [3.0, -2.0], np.full(20, -30.0) + rng.normal(0, 0.01, 20)])
        if k % 3 == 0:
            pw[:, 2] += 0.5                                  # a third of the observers see the patch half a metre off
        pb = ((pw - tr) @ R).astype(np.float32).astype(np.float64)
        out.append(np.concatenate([[np.sum(pb[:, 0] * pb[:, 0]), np.sum(pb[:, 0] * pb[:, 1]), np.sum(pb[:, 0] * pb[:, 2]),
                                    np.sum(pb[:, 1] * pb[:, 1]), np.sum(pb[:, 1] * pb[:, 2]), np.sum(pb[:, 2] * pb[:, 2])],
                                   pb.sum(0), [20.0]]))
    V = len(off) - 1
    h = V // 2
    new_off = np.concatenate([off[:h + 1], [off[h] + 280], off[h + 1:] + 280]).astype(np.int64)
    new_idx = np.concatenate([idx[:off[h]], poses.astype(np.int32), idx[off[h]:]]).astype(np.int32)
    new_clu = np.concatenate([clu[:off[h]], np.asarray(out), clu[off[h]:]])
    dd = dict(d, voxel_off=new_off, pose_idx=new_idx, clusters=new_clu)
    a = rbo.derive_scale(d, d["poses_init"])
    x0 = d["poses_init"]
    prob = rbo.problem(dd)
    Ho, go, co_, lam, w = rbo.evaluate(prob, x0, "cauchy", a)
    assert lam[h] > a * a and w[h] < 0.5                     # the big voxel is an outlier at this scale
    p = _prob(pkg, dd)
    p.set_loss(("cauchy", a))
    c = p.cost(x0)
    H, g, ca = p.eval(x0)
    assert abs(c - co_) <= 1e-8 * co_ and rel(g, go) <= 1e-8 and rel(H, Ho) <= 1e-8
    assert p.cost(x0, is_avg=True) == ca
    lg, wg = p.voxel_residuals(x0)
    assert abs(lg[h] - lam[h]) <= 1e-8 * lam[h] and abs(wg[h] - w[h]) <= 1e-8
    p.close()


def test_y32_records_with_a_loss(pkg, monkeypatch):
    """LVBA_Y32=1 (fp32 Y records between the factor and the pair pass) with a loss, at that mode's existing bars
    (tests/test_gpu_balm.py::test_y32_switch_keeps_cost_gradient_and_lm_trace): cost, gradient and diagonal blocks bitwise equal
    to the fp64-record run, off-diagonal blocks within 5e-6; and the cost against the oracle."""
    d = make_problem(300, 60000, seed=9)
    a = rbo.derive_scale(d, d["poses_init"])
    dc, _ = rbo.add_outlier_voxels(d, 0.25, 10, 5 * a, 20 * a)
    rbo.check_input_shares(dc, a)
    x0 = dc["poses_init"]
    monkeypatch.setenv("LVBA_PAIR_WINDOW", "4096")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("LVBA_Y32", mode)
        p = _prob(pkg, dc)
        p.set_loss(("cauchy", a))
        assert p.info()["y_fp32"] == int(mode)
        out[mode] = p.eval(x0)
        p.close()
    (H0, g0, c0), (H1, g1, c1) = out["0"], out["1"]
    co_ = rbo.cost(rbo.problem(dc), x0, "cauchy", a)
    assert abs(c0 * 60000 - co_) <= 1e-8 * co_
    assert c1 == c0 and np.array_equal(g1, g0)
    Hb0, Hb1 = H0.reshape(300, 6, 300, 6), H1.reshape(300, 6, 300, 6)
    for i in range(300):
        assert np.array_equal(Hb0[i, :, i, :], Hb1[i, :, i, :])
    assert not np.array_equal(H1, H0) and rel(H1, H0) <= 5e-6 and np.array_equal(H1, H1.T)
    # and directly against the oracle composition, on a problem small enough for it whose pair lists are windowed too (the
    # column pair kernel, where the switch applies): cost and g from fp64 registers at 1e-8, H at the mode's 5e-6
    _, dm, _, am = _inputs(MID)
    monkeypatch.setenv("LVBA_PAIR_WINDOW", "256")
    monkeypatch.setenv("LVBA_Y32", "1")
    Ho, go, co_, _, _ = rbo.evaluate(rbo.problem(dm), dm["poses_init"], "cauchy", am)
    p = _prob(pkg, dm)
    p.set_loss(("cauchy", am))
    assert p.info()["y_fp32"] == 1
    H, g, c = p.eval(dm["poses_init"])
    print(f"Y32 vs oracle: cost {abs(c * p.n_voxels - co_) / co_:.2e} g {rel(g, go):.2e} H {rel(H, Ho):.2e}")
    assert abs(c * p.n_voxels - co_) <= 1e-8 * co_ and rel(g, go) <= 1e-8
    assert rel(H, Ho) <= 5e-6 and rel(H, Ho) > 1e-10          # (fp32 records did take effect)
    p.close()


def test_voxel_residuals_in_caller_order_after_a_relayout(pkg):
    """A problem large enough for the internal voxel re-layout (300 poses, 60 000 voxels) with its voxels SHUFFLED, so that the
    re-layout triggers: lambda_min and the weights come back in the caller's (shuffled) order.  Also the small problem, where
    no re-layout happens; each problem with the scale derived from it.
    Bar on lambda_min, PER VOXEL: 1e-8 lambda + 16 eps M_v, M_v = robust_balm_oracle.voxel_moment_scale (the largest
    (|p_f| + |v_f| / n_f)^2 over the voxel's factors).  The absolute floor is what fp64 leaves of the formula both sides use, the
    pose transform of the second moments followed by C = S / N - vbar vbar^T: the terms are of size M_v per point, an entry
    reaches the subtraction through ~3 roundings (transform, sum over the factors, division) of eps M_v / 2 each, lambda_min
    moves by at most the 2-norm of the 3 x 3 perturbation (Weyl; <= 3 x the largest entry), and two implementations are compared:
    2 x 3 x 3 x eps / 2 ~ 9 eps M_v, rounded up to 16.  On the 300-pose problem M_v is 1e3 .. 1.3e5 m^2, the floor 4e-12 .. 5e-10
    against lambda ~ 1e-4 of an inlier, so a pure 1e-8 lambda is not reachable there: the oracle's OWN error against an
    80-bit evaluation of the same formula is up to 6.4e-8 lambda (1.4 eps M_v) on this problem.  The test prints the worst
    ratios."""
    d = make_problem(300, 60000, seed=9)
    a = rbo.derive_scale(d, d["poses_init"])
    dc, _ = rbo.add_outlier_voxels(d, 0.25, 10, 5 * a, 20 * a)
    rbo.check_input_shares(dc, a)
    off, idx, clu = dc["voxel_off"], dc["pose_idx"], dc["clusters"].reshape(-1, 10)
    V = len(off) - 1
    order = np.random.default_rng(3).permutation(V)
    k = np.diff(off)
    new_off = np.concatenate([[0], np.cumsum(k[order])]).astype(np.int64)
    gather = np.concatenate([np.arange(off[v], off[v + 1]) for v in order])
    ds = dict(dc, voxel_off=new_off, pose_idx=idx[gather], clusters=clu[gather])
    _, dsmall, _, a_small = _inputs(SMALL)
    for dd, a in ((ds, a), (dsmall, a_small)):
        x0 = dd["poses_init"]
        M = rbo.voxel_moment_scale(rbo.problem(dd), x0)
        for kind in ("cauchy", "tukey"):
            lam, w = rbo.lambdas_weights(rbo.problem(dd), x0, kind, a)
            p = _prob(pkg, dd)
            p.set_loss((kind, a))
            lg, wg = p.voxel_residuals(x0)
            dl = np.abs(lg - lam)
            eps = np.finfo(np.float64).eps
            print(f"V={len(lam)} {kind}: worst |dlam|/lam {np.max(dl / lam):.2e}, worst |dlam|/(eps M) {np.max(dl / (eps * M)):.2f}, "
                  f"M up to {M.max():.3g}, worst |dlam|/(1e-8 lam + 16 eps M) {np.max(dl / (1e-8 * lam + 16 * eps * M)):.3f}")
            assert (dl <= 1e-8 * lam + 16 * eps * M).all()
            assert np.abs(wg - w).max() <= 1e-8
            assert wg.min() < 0.5 and wg.max() > 0.9
            p.close()


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_refinement_matches_the_oracle_lm(pkg, kind):
    d, dc, _, a = _inputs(SMALL)
    x0 = dc["poses_init"]
    xo, tro = rbo.damping_iter(rbo.problem(dc), x0, kind, a)
    p = _prob(pkg, dc)
    p.set_loss((kind, a))
    x, tr, rc = p.refine(x0)
    assert rc == 0
    _compare_traces(tr, _rows(tro), x, xo)
    # the reason the feature exists: closer to the uncontaminated solution than the plain LM ends
    q = _prob(pkg, dc)
    x_plain, _, _ = q.refine(x0)
    c = _prob(pkg, d)
    x_clean, _, _ = c.refine(d["poses_init"])
    d_plain, d_rob = rbo.gauge_distance(x_plain, x_clean), rbo.gauge_distance(x, x_clean)
    print(f"{kind}: plain {d_plain:.4f} m, robust {d_rob:.4f} m")
    assert d_rob < d_plain
    for h in (p, q, c):
        h.close()


def test_grouped_handle_equals_each_window_alone(pkg):
    parts, scales = [], []
    for case in (MID, SMALL):                                 # two windows of different size
        dc, _, a = rbo.contaminated(make_problem(**case))
        parts.append(dc); scales.append(a)
    a = min(scales)                                           # one loss for the handle
    for dc in parts:
        rbo.check_input_shares(dc, a)
    pose_off = np.cumsum([0] + [d["n_poses"] for d in parts]).astype(np.int32)
    vox_off = np.cumsum([0] + [len(d["voxel_off"]) - 1 for d in parts]).astype(np.int64)
    off, idx, clu = [np.zeros(1, np.int64)], [], []
    for k, d in enumerate(parts):
        off.append(d["voxel_off"][1:] + off[-1][-1])
        idx.append(d["pose_idx"] + pose_off[k])
        clu.append(d["clusters"].reshape(-1, 10))
    off, idx, clu = np.concatenate(off), np.concatenate(idx).astype(np.int32), np.concatenate(clu)
    x0 = np.concatenate([d["poses_init"] for d in parts])
    u = pkg.BalmProblem(int(pose_off[-1]), off, idx, clu)
    u.set_groups(pose_off, vox_off)
    u.set_loss(("cauchy", a))
    xu, per, rc = u.refine_groups(x0)
    assert rc == 0
    for k, d in enumerate(parts):
        p = _prob(pkg, d)
        p.set_loss(("cauchy", a))
        xs, tr, rck = p.refine(d["poses_init"])
        plain = _prob(pkg, d)
        assert tr[0]["residual1"] < plain.cost(d["poses_init"], is_avg=True)     # the loss is in effect
        assert rck == 0 and per["n_iter"][k] == len(tr)
        assert abs(per["cost_first"][k] - tr[0]["residual1"]) <= 1e-9 * tr[0]["residual1"]
        last = tr[-1]["residual2"] if tr[-1]["accepted"] else tr[-1]["residual1"]
        assert abs(per["cost_last"][k] - last) <= 1e-8 * last
        assert np.abs(xu[pose_off[k]:pose_off[k + 1]] - xs).max() <= 1e-8, k
        p.close(); plain.close()
    u.close()


def _priors(d):
    x = d["poses_gt"].reshape(-1, 12)
    N = x.shape[0]
    L6 = np.diag([40.0, 30.0, 20.0, 6.0, 4.0, 2.0])
    rng = np.random.default_rng(0)
    out = [po.make_prior("pose", 0, np.r_[x[0, :9], x[0, 9:] + rng.normal(scale=0.01, size=3)], L6)]
    for i in range(3, N, 4):
        out.append(po.make_prior("position", i, np.r_[np.eye(3).reshape(9), x[i, 9:] + rng.normal(scale=0.02, size=3)],
                                 np.diag([5.0, 5.0, 3.0, 0, 0, 0])))
    return out


def _set(pkg, p, priors):
    p.set_priors([pkg.Prior._make({0: "pose", 1: "position", 2: "relative"}[q["kind"]], q["i"], q["j"], q["meas"], q["L"],
                                  q["oi"], q["oj"]) for q in priors])


def test_priors_stay_outside_the_loss(pkg):
    _, dc, _, a = _inputs(SMALL)
    x0 = dc["poses_init"]
    priors = _priors(dc)
    p = _prob(pkg, dc)
    _set(pkg, p, priors)
    e0, cp0 = p.prior_residuals(x0)
    p.set_loss(("cauchy", a))
    e1, cp1 = p.prior_residuals(x0)
    assert np.array_equal(e0, e1) and cp0 == cp1
    cv = rbo.cost(rbo.problem(dc), x0, "cauchy", a)
    cpo = po.assemble(priors, x0)[2]
    assert abs(cp1 - cpo) <= 1e-8 * cpo
    c = p.cost(x0)
    assert abs(c - (cv + cpo)) <= 1e-8 * (cv + cpo)
    xo, tro = rbo.damping_iter(rbo.problem(dc), x0, "cauchy", a, priors=priors)
    x, tr, rc = p.refine(x0)
    assert rc == 0
    _compare_traces(tr, _rows(tro), x, xo)
    p.close()


def test_covariance_is_the_inverse_of_the_robust_hessian(pkg):
    import cov_oracle as co
    from test_gpu_covariance import _pairs_of, _worst
    _, dc, _, a = _inputs(MID)
    x = np.ascontiguousarray(dc["poses_gt"], np.float64).reshape(-1, 12)
    N = dc["n_poses"]
    Ho = rbo.evaluate(rbo.problem(dc), x, "cauchy", a)[0]
    p = _prob(pkg, dc)
    p.set_loss(("cauchy", a))
    pairs, _ = _pairs_of(p, x)
    for anchor in (0, N // 2):
        diag, pb, av = p.covariance(x, anchor=anchor, pairs=pairs)
        assert np.all(diag[anchor] == 0.0)
        wd, wp = _worst(co.anchored_inverse(Ho, anchor), diag, pairs, pb, av)
        print(f"anchor {anchor}: diag {wd:.2e}, pairs {wp:.2e}")
        assert wd <= 1e-8 and wp <= 1e-8
    p.close()


def test_two_ranks_equal_one_and_refuse_different_losses(pkg):
    _, dc, _, a = _inputs(MID)
    N, off, idx, clu = dc["n_poses"], dc["voxel_off"], dc["pose_idx"], dc["clusters"].reshape(-1, 10)
    V = len(off) - 1
    x0 = dc["poses_init"]
    one = _prob(pkg, dc)
    one.set_loss(("cauchy", a))
    H1, g1, c1 = one.eval(x0)
    x1, tr1, rc1 = one.refine(x0)
    lam1, w1 = one.voxel_residuals(x0)
    one.close()

    def run(scales):
        ht = HostTransport(2)

        def rank_main(r):
            lo, hi = pkg.shard_range(V, r, 2)
            q = pkg.BalmProblem(N, off[lo:hi + 1], idx[off[lo]:off[hi]], clu[off[lo]:off[hi]])
            ht.attach(q, r)
            q.set_loss(("cauchy", scales[r]))
            try:
                H, g, c = q.eval(x0)
                x, tr, rc = q.refine(x0)
                lam, w = q.voxel_residuals(x0)
                return dict(H=H, g=g, c=c, x=x, tr=tr, rc=rc, lam=lam, w=w, lo=lo, hi=hi)
            except pkg._lib.LvbaError as e:
                return e.code
            finally:
                q.close()

        return ht.run(rank_main)

    out = run([a, a])
    r0, r1 = out
    assert np.array_equal(r0["H"], r1["H"]) and np.array_equal(r0["x"], r1["x"]) and r0["tr"] == r1["tr"]
    assert rel(r0["H"], H1) <= 1e-12 and rel(r0["g"], g1) <= 1e-12 and abs(r0["c"] - c1) <= 1e-12 * c1
    assert r0["rc"] == rc1 == 0 and len(r0["tr"]) == len(tr1)
    for u, v in zip(r0["tr"], tr1):
        assert u["accepted"] == v["accepted"] and abs(u["residual2"] - v["residual2"]) <= 1e-7 * v["residual2"]
    assert np.abs(r0["x"] - x1).max() <= 1e-8
    for r in out:                                             # voxel_residuals is rank-local: the shard's voxels
        assert np.array_equal(r["lam"], lam1[r["lo"]:r["hi"]]) and np.array_equal(r["w"], w1[r["lo"]:r["hi"]])
    assert run([a, 2.0 * a]) == [pkg._lib.ERR_ARG] * 2


def test_argument_errors_leave_the_handle_working(pkg):
    L = pkg._lib
    _, dc, _, a = _inputs(SMALL)
    x0 = dc["poses_init"]
    p = _prob(pkg, dc)
    p.set_loss(("cauchy", a))
    c = p.cost(x0)
    for bad in ((17, a), (-1, a), ("huber", 0.0), ("cauchy", -1.0), ("tukey", float("nan")), ("huber", float("inf"))):
        with pytest.raises(L.LvbaError) as e:
            p.set_loss(bad)
        assert e.value.code == L.ERR_ARG
        assert p.cost(x0) == c                                # unchanged
    with pytest.raises(ValueError):
        p.set_loss(("no such loss", 1.0))
    p.lm_begin(x0)
    with pytest.raises(L.LvbaError) as e:
        p.set_loss(None)
    assert e.value.code == L.ERR_STATE
    done = False
    while not done:
        _, done, _ = p.lm_step()
    x = p.lm_end()
    x2, _, _ = p.refine(x0)
    assert np.array_equal(x, x2)
    p.set_loss(None)                                          # allowed again
    q = _prob(pkg, dc)
    assert p.cost(x0) == q.cost(x0)
    p.close(); q.close()


def _scans(synth):
    return synth.make_scans(24, 80000, room=(14, 10, 4), n_panels=0, n_blobs=0, clutter_frac=0.0, seed=61, rot_sigma_deg=0.15,
                            trans_sigma=0.04)


def test_whole_stage_entry(pkg, synth):
    """lvba_lidar_ba_robust: both losses NULL is lvba_lidar_ba bit for bit; with a stage loss it equals the host-driven flow of
    pipeline.run_lidar_ba, which sets the loss through BalmProblem.set_loss; with a window loss the window stage changes."""
    import ctypes as C
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    L = pkg._lib
    s = _scans(synth)
    x0 = np.asarray(s["poses"], np.float64).reshape(-1, 12)
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    with pkg.Scans(s["clouds"]) as sc:
        xa, ra = pipe.run_lidar_ba(sc, x0, **cfg)
        # both losses NULL, through the new entry itself
        o = L.LidarBaOpts()
        sc.lib.lvba_lidar_ba_default_opts(C.byref(o))
        o.window.window_size, o.window.anchor_leaf = 6, 0.02
        o.window.voxel.voxel_size = 1.0
        for i, (vs, er) in enumerate(zip(cfg["stage_voxel_size"], cfg["stage_eigen_ratio"])):
            o.stage_voxel_size[i] = vs
            for k in range(4):
                o.stage_eigen_ratio[i][k] = er[k]
        out, rep = np.zeros(x0.size), L.LidarBaReport()
        hs = (C.c_void_p * 1)(sc._h.value)
        L.check(sc.lib.lvba_lidar_ba_robust(1, hs, x0.reshape(-1), C.byref(o), None, None, 0, None, out, C.byref(rep), None, None, None))
        assert np.array_equal(out.reshape(-1, 12), xa) and rep.as_dict()["stage_iters"] == ra["stage_iters"]
        assert ra["stage_ran"][1] == 1
        loss = ("cauchy", 0.05)
        xb, rb = pipe.run_lidar_ba(sc, x0, stage_loss=loss, **cfg)
        xh, rh = pipe.run_lidar_ba(sc, x0, stage_loss=loss, host_driven=True, **cfg)
        assert not np.array_equal(xb, xa)
        assert list(rb["stage_iters"]) == list(rh["stage_iters"])
        assert np.abs(xb - xh).max() <= 1e-9
        xw, _ = pipe.run_lidar_ba(sc, x0, window_loss=loss, **cfg)
        assert not np.array_equal(xw, xa)
        with pytest.raises(L.LvbaError) as e:
            pipe.run_lidar_ba(sc, x0, stage_loss=("huber", -1.0), **cfg)
        assert e.value.code == L.ERR_ARG


def test_whole_stage_entry_over_two_shares(pkg, synth):
    """lvba_lidar_ba_robust with n_shares = 2 (both on device 0): the window loss travels through the multi-share window stage.
    Against the one-share call with the same losses at the bar tests/test_gpu_window.py holds the two without a loss (the grouped
    window LM sees other groups per share: rounding-level differences that the stages amplify)."""
    s = synth.make_scans(16, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=43, rot_sigma_deg=0.1, trans_sigma=0.03)
    kw = dict(window_size=4, anchor_leaf=0.05, stage_voxel_size=(1.0, 0.5))
    loss = dict(window_loss=("cauchy", 0.05), stage_loss=("huber", 0.05))
    with pkg.Scans(s["clouds"]) as scans:
        one, rep1 = scans.lidar_ba(s["poses"], **kw, **loss)
        one_w, _ = scans.lidar_ba(s["poses"], window_loss=loss["window_loss"], **kw)
        plain, _ = scans.lidar_ba(s["poses"], **kw)
    two, rep2 = pkg.Scans.lidar_ba_multi(s["clouds"], s["poses"], (0, 0), **kw, **loss)
    two_w, _ = pkg.Scans.lidar_ba_multi(s["clouds"], s["poses"], (0, 0), window_loss=loss["window_loss"], **kw)
    two_plain, _ = pkg.Scans.lidar_ba_multi(s["clouds"], s["poses"], (0, 0), **kw)
    assert rep2["n_windows"] == rep1["n_windows"] == 4 and rep2["n_anchors"] == rep1["n_anchors"] == 4
    assert np.abs(two - one).max() < 2e-4 and np.abs(two_w - one_w).max() < 2e-4
    assert not np.array_equal(two_w, two_plain) and not np.array_equal(two, two_w)     # each loss reaches its stage
    assert not np.array_equal(one, plain)
    # the report's form follows `priors is not None`, with or without a loss
    with pkg.Scans(s["clouds"]) as scans:
        _, r_none = scans.lidar_ba(s["poses"], stage_loss=loss["stage_loss"], **kw)
        _, r_empty = scans.lidar_ba(s["poses"], priors=[], stage_loss=loss["stage_loss"], **kw)
    assert "priors_used" not in r_none and r_empty["priors_used"] == 0
