"""GPU tests of the marginal pose covariance (lvba_balm_covariance): every case held against a dense numpy inverse of the Hessian
(from the C oracle, with the priors of tests/prior_oracle.py, or downloaded from the handle), the refusals, the absence of side
effects on the handle, and ranks."""
import numpy as np
import pytest

import cov_oracle as co
import prior_oracle as po
from conftest import HostTransport, make_problem
from cov_oracle import worst as _worst

pytestmark = pytest.mark.gpu

BAND = dict(n_poses=600, n_voxels=30000, band=10, seed=3)
SMALL = dict(n_poses=150, n_voxels=8000, band=12, seed=4)    # (a ring: the store is dense)
TINY = dict(n_poses=9, n_voxels=800, band=3, seed=1)
ND = dict(n_poses=320, n_voxels=16000, band=12, seed=3, revisit="lot")


def _prob(pkg, d, priors=None, **kw):
    p = pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"], **kw)
    if priors is not None:
        p.set_priors([pkg.Prior._make({0: "pose", 1: "position", 2: "relative"}[q["kind"]], q["i"], q["j"], q["meas"], q["L"],
                                      q["oi"], q["oj"]) for q in priors])
    return p


def _rel_gt(x, i, j):
    Ri, pi_ = x[i, :9].reshape(3, 3), x[i, 9:]
    Rj, pj = x[j, :9].reshape(3, 3), x[j, 9:]
    return np.r_[(Ri.T @ Rj).reshape(9), Ri.T @ (pj - pi_)]


def _mix(d, seed=0, loop=True):
    """POSE on pose 0, POSITION with a lever arm on every 10th pose, RELATIVE on every 7th consecutive pair and, with loop, one
    joining the two ends (tests/test_gpu_priors.py's set)"""
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
        a, b = (i + 1, i) if i % 2 else (i, i + 1)
        m = _rel_gt(x, a, b)
        m[:9] = (m[:9].reshape(3, 3) @ po.so3_exp(rng.normal(scale=1e-3, size=3))).reshape(9)
        m[9:] += rng.normal(scale=0.005, size=3)
        out.append(po.make_prior("relative", a, m, L6, j=b))
    if loop:
        out.append(po.make_prior("relative", N - 1, _rel_gt(x, N - 1, 0), L6, j=0,
                                 oi=np.r_[po.so3_exp([0.0, 0.3, 0.0]).reshape(9), 0.0, 0.5, 0.0],
                                 oj=np.r_[po.so3_exp([0.0, 0.3, 0.0]).reshape(9), 0.0, 0.5, 0.0]))
    return out


def _dense_from_blocks(N, bi, bj, blocks):
    H = np.zeros((6 * N, 6 * N))
    for i, j, b in zip(bi, bj, blocks):
        H[6 * i:6 * i + 6, 6 * j:6 * j + 6] = b
        H[6 * j:6 * j + 6, 6 * i:6 * i + 6] = b.T
    return H


def _refined(p, d, iters=30):
    x, _, rc = p.refine(d["poses_init"], max_iter=iters)
    assert rc == 0
    return x


def _gt(d):
    """the ground-truth poses: H is positive definite there once the gauge is fixed (a refinement of the synthetic problems can end
    beside a voxel whose lambda_min is not locally convex, where H has a negative eigenvalue and the covariance is refused)"""
    return np.ascontiguousarray(d["poses_gt"], np.float64).reshape(-1, 12)


def _pairs_of(p, x):
    bi, bj, blocks, _, _ = p.eval_blocks(x)
    off = bi != bj
    return np.stack([bi[off], bj[off]], 1), (bi, bj, blocks)


@pytest.mark.parametrize("case,kw", [(BAND, {}), (SMALL, dict(band_frac=0.0)), (TINY, dict(band_frac=0.0))],
                         ids=["band", "dense", "dense-single-panel"])
def test_anchored_covariance_matches_the_dense_inverse(pkg, oracle_mod, case, kw):
    d = make_problem(**case)
    N = d["n_poses"]
    p = _prob(pkg, d, **kw)
    info = p.info()
    assert info["use_band"] == (0 if kw else 1)
    if not kw:
        assert not np.array_equal(p.ordering(), np.arange(N))    # the internal order is not the caller's
        assert 6 * N > 64 * 8 and (6 * N) % 64 != 0             # many panels, a partial last one
    x = _gt(d)
    pairs, (bi, bj, blocks) = _pairs_of(p, x)
    Hg = _dense_from_blocks(N, bi, bj, blocks)
    Ho, _, _ = oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"]).eval_dense(x)
    for anchor in (0, N // 2, N - 1):
        diag, pb, av = p.covariance(x, anchor=anchor, pairs=pairs)
        assert av.all()                                         # every pair that shares a voxel lies in the band
        assert np.all(diag[anchor] == 0.0)
        for name, H in (("oracle", Ho), ("gpu H", Hg)):
            wd, wp = _worst(co.anchored_inverse(H, anchor), diag, pairs, pb, av)
            print(f"anchor {anchor} vs inv({name}): diag {wd:.2e}, pairs {wp:.2e}")
            assert wd <= 1e-8 and wp <= 1e-8, (name, anchor, wd, wp)


@pytest.mark.parametrize("loop", [False, True], ids=["band", "loop-closure"])
def test_priors_fix_the_gauge(pkg, oracle_mod, loop):
    d = make_problem(**SMALL)
    N = d["n_poses"]
    priors = _mix(d, loop=loop)
    p = _prob(pkg, d, priors)
    print("priors: use_band", p.info()["use_band"], "band_blocks", p.info()["band_blocks"])
    x = _gt(d)
    orc = po.PriorOracle(oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"]), priors)
    H, _, _ = orc.eval_dense(x)
    pairs, _ = _pairs_of(p, x)
    relp = np.array([[q["i"], q["j"]] for q in priors if q["kind"] == 2])
    allp = np.concatenate([pairs, relp])
    diag, pb, av = p.covariance(x, pairs=allp)
    assert av.all()                                              # relative priors are edges of the band too
    wd, wp = _worst(co.inv(H), diag, allp, pb, av)
    print(f"priors vs inv(H + H_priors): diag {wd:.2e}, pairs {wp:.2e}")
    assert wd <= 1e-8 and wp <= 1e-8
    for b in diag:                                               # symmetric, positive definite
        assert np.array_equal(b, b.T)
        assert np.linalg.eigvalsh(b).min() > 0


def test_stiff_pose_prior_matches_the_anchor(pkg):
    d = make_problem(**SMALL)
    N, k = d["n_poses"], 40
    p = _prob(pkg, d)
    x = _gt(d)
    da, _, _ = p.covariance(x, anchor=k)
    stiff = [po.make_prior("pose", k, x[k], 1e6 * np.eye(6))]
    q = _prob(pkg, d, stiff)
    dp, _, _ = q.covariance(x)
    keep = np.arange(N) != k
    err = max(np.linalg.norm(dp[i] - da[i]) / np.linalg.norm(da[i]) for i in np.nonzero(keep)[0])
    print(f"stiff POSE prior vs anchor: {err:.2e}")
    assert err <= 1e-6
    assert np.linalg.norm(dp[k]) <= 1e-6 * max(np.linalg.norm(da[i]) for i in np.nonzero(keep)[0])


def test_free_gauge_is_refused_and_harmless(pkg):
    d = make_problem(**SMALL)
    p = _prob(pkg, d)
    diag = np.full((d["n_poses"], 6, 6), 7.0)
    with pytest.raises(pkg._lib.LvbaError) as e:
        import ctypes as C
        o = pkg._lib.CovOpts()
        p.lib.lvba_cov_default_opts(C.byref(o))
        pkg._lib.check(p.lib.lvba_balm_covariance(p._h, p._poses(d["poses_init"]), C.byref(o), diag.ctypes.data, 0, None, None, None,
                                                  None))
    assert e.value.code == pkg._lib.NUM_FACTORIZATION
    assert np.all(diag == 7.0)                                   # nothing written
    x1, t1, rc1 = p.refine(d["poses_init"])
    x2, t2, rc2 = _prob(pkg, d).refine(d["poses_init"])
    assert rc1 == rc2 == 0 and x1.tobytes() == x2.tobytes() and t1 == t2


def test_refusals(pkg, monkeypatch):
    d = make_problem(**SMALL)
    N = d["n_poses"]
    p = _prob(pkg, d)
    x = d["poses_init"]
    E = pkg._lib
    for kw in (dict(anchor=N), dict(anchor=-2), dict(anchor=0, pairs=[[3, 3]]), dict(anchor=0, pairs=[[0, N]]),
               dict(anchor=0, pairs=[[-1, 2]])):
        with pytest.raises(E.LvbaError) as e:
            p.covariance(x, **kw)
        assert e.value.code == E.ERR_ARG, kw
    p.lm_begin(x)
    with pytest.raises(E.LvbaError) as e:
        p.covariance(x, anchor=0)
    assert e.value.code == E.ERR_STATE
    p.lm_end()
    # groups need every voxel inside one group: build a two-group problem from two independent copies of a small problem
    t = make_problem(**TINY)
    tv, tp, tc, tn = np.asarray(t["voxel_off"]), np.asarray(t["pose_idx"]), np.asarray(t["clusters"]), t["n_poses"]
    voff = np.concatenate([tv, tv[1:] + tv[-1]])
    gp = pkg.BalmProblem(2 * tn, voff, np.concatenate([tp, tp + tn]), np.concatenate([tc, tc]))
    gp.set_groups([0, tn, 2 * tn], [0, len(tv) - 1, 2 * (len(tv) - 1)])
    with pytest.raises(E.LvbaError) as e:
        gp.covariance(np.concatenate([t["poses_init"], t["poses_init"]]), anchor=0)
    assert e.value.code == E.ERR_UNSUPPORTED
    monkeypatch.setenv("LVBA_SOLVER", "nd")
    dn = make_problem(**ND)
    q = _prob(pkg, dn)
    q.cost(dn["poses_init"])
    assert q.info()["nd_kind"] != 0
    with pytest.raises(E.LvbaError) as e:
        q.covariance(dn["poses_init"], anchor=0)
    assert e.value.code == E.ERR_UNSUPPORTED


def test_pairs_outside_the_band(pkg):
    d = make_problem(**BAND)
    N = d["n_poses"]
    p = _prob(pkg, d)
    x = _gt(d)
    perm = p.ordering()
    Bb = p.info()["band_blocks"]
    far = [perm[0], perm[N - 1]]
    near = [perm[5], perm[5 + Bb]]
    diag, pb, av = p.covariance(x, anchor=0, pairs=[far, near])
    assert list(av) == [False, True]
    assert np.isnan(pb[0]).all() and np.isfinite(pb[1]).all()


@pytest.mark.parametrize("case", [BAND, SMALL], ids=["band", "dense"])
def test_no_side_effects(pkg, case):
    d = make_problem(**case)
    a, b = _prob(pkg, d), _prob(pkg, d)
    xa = _refined(a, d)
    xb = _refined(b, d)
    assert xa.tobytes() == xb.tobytes()
    x = _gt(d)
    pairs, _ = _pairs_of(a, x)
    c1 = a.covariance(x, anchor=3, pairs=pairs)
    c2 = a.covariance(x, anchor=3, pairs=pairs)
    for u, v in zip(c1, c2):
        assert u.tobytes() == v.tobytes()                        # two calls: the same bits
    for h in (a, b):
        h.eval(xa, want_H=False)
    assert a.solve(0.01).tobytes() == b.solve(0.01).tobytes()
    ya = a.refine(d["poses_init"])
    yb = b.refine(d["poses_init"])
    assert ya[0].tobytes() == yb[0].tobytes() and ya[1] == yb[1]


def test_ranks_agree(pkg):
    d = make_problem(**BAND)
    N, off, idx, clu = d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]
    V = len(off) - 1
    p = _prob(pkg, d)
    assert p.info()["use_band"] == 1
    x = _gt(d)
    pairs, _ = _pairs_of(p, x)
    ref = p.covariance(x, anchor=7, pairs=pairs)
    ht = HostTransport(2)

    def rank_main(r):
        lo, hi = pkg.shard_range(V, r, 2)
        q = pkg.BalmProblem(N, off[lo:hi + 1], idx[off[lo]:off[hi]], clu[off[lo]:off[hi]])
        ht.attach(q, r)
        out = q.covariance(x, anchor=7, pairs=pairs)
        q.close()
        return out

    out = ht.run(rank_main)
    for u, v in zip(out[0], out[1]):
        assert u.tobytes() == v.tobytes()
    assert np.array_equal(out[0][2], ref[2])
    for u, v in zip(out[0][:2], ref[:2]):
        assert np.abs(u - v).max() <= 1e-12 * np.abs(v).max()
