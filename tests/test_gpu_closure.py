"""GPU tests of the pairwise consistency of loop closures: lvba_closure_consistency against the numpy restatement
(tests/closure_oracle.py) on the shared cases (tests/closure_cases.py), its argument checks, pipeline.consistent_closures and
pipeline.find_loop_closures(consistency=...) on the fixtures of §10d and §10e."""
import ctypes as C
import importlib

import numpy as np
import pytest

import closure_cases as cc
import closure_oracle as co
import loop_cases as lc
import place_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("global-lvba_amd.register")


@pytest.fixture(scope="module")
def pl(pkg):
    return importlib.import_module("global-lvba_amd.pipeline")


def run(reg, c, **kw):
    return reg.closure_consistency(c["X"], c["ref"], c["query"], c["Z"], **dict(c["opts"], **kw))


@pytest.mark.parametrize("k", range(len(cc.cases())), ids=[c["name"] for c in cc.cases()])
def test_consistency_equals_the_oracle(reg, k):
    """Adjacency bytes and keep are the oracle's, rot / trans within 1e-9 of it (the bar of tests/test_closure_host.py); two calls
    give the same bytes; without the optional outputs keep is the same."""
    c = cc.cases()[k]
    adj, g = cc.oracle(k)
    M = len(c["Z"])
    got = run(reg, c, diagnostics=True)
    err = max(np.abs(got["rot"] - adj["rot"]).max(initial=0.0), np.abs(got["trans"] - adj["trans"]).max(initial=0.0))
    print(f"{c['name']}: kept {got['n_keep']} of {M}, largest |rot, trans - oracle| {err:.2e}")
    assert got["words"].tobytes() == co.words(adj["rows"], M).tobytes()
    assert got["keep"].tolist() == g["keep"] and got["n_keep"] == g["n_keep"]
    assert err <= 1e-9
    assert np.array_equal(got["adjacency"], co.dense(adj["rows"], M)) and got["adjacency"].shape == (M, M)
    again = run(reg, c, diagnostics=True)
    assert all(again[f].tobytes() == got[f].tobytes() for f in ("words", "keep", "rot", "trans")) and again["n_keep"] == got["n_keep"]
    # NULL adjacency / rot / trans
    L = importlib.import_module("global-lvba_amd._lib")
    keep, n_keep = np.full(max(M, 1), 9, np.uint8), C.c_int32(-1)
    o = L.ClosureOpts(**c["opts"])
    ptr = lambda a: a.ctypes.data if M else None
    assert L.load().lvba_closure_consistency(0, len(c["X"]), c["X"].ctypes.data, M, ptr(c["ref"]), ptr(c["query"]), ptr(c["Z"]), C.byref(o),
                                             None, None, None, keep.ctypes.data, C.byref(n_keep)) == L.OK
    assert n_keep.value == g["n_keep"] and keep[:M].astype(bool).tolist() == g["keep"]


def test_defaults_and_bad_arguments(pkg, reg):
    L = pkg._lib
    lib = L.load()
    o = L.ClosureOpts()
    lib.lvba_closure_default_opts(C.byref(o))
    assert (o.rot_tol, o.rot_rate, o.trans_tol, o.trans_rate, o.n_seeds, o.min_set) == tuple(co.DEFAULTS[k] for k in (*co.TOLS, "n_seeds", "min_set"))
    c = cc.named("two cliques")
    want = cc.oracle([x["name"] for x in cc.cases()].index("two cliques"))[1]
    X, ref, query, Z = c["X"].copy(), c["ref"].copy(), c["query"].copy(), c["Z"].copy()
    M, nf = len(Z), len(X)
    keep, n_keep = np.full(M, 7, np.uint8), C.c_int32(-5)
    words, rot, trans = np.full((M, 1), 0xABCD, np.uint64), np.full((M, M), -3.0), np.full((M, M), -4.0)

    def call(n_frames=nf, X=X, n=M, ref=ref, query=query, Z=Z, opts=None, keep=keep, n_keep=n_keep):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.lvba_closure_consistency(0, n_frames, p(X), n, p(ref), p(query), p(Z), None if opts is None else C.byref(opts), p(words),
                                            p(rot), p(trans), p(keep), None if n_keep is None else C.byref(n_keep))

    def refused(rc):
        assert rc == L.ERR_ARG and lib.lvba_last_error()
        assert n_keep.value == -5 and (keep == 7).all() and (words == 0xABCD).all() and (rot == -3.0).all() and (trans == -4.0).all()

    for missing in ("X", "ref", "query", "Z", "keep", "n_keep"):
        refused(call(**{missing: None}))
    refused(call(n=-1))
    refused(call(n=16385))
    refused(call(n_frames=0))
    refused(call(n_frames=int(query.max())))                       # an index outside the frames
    bad = ref.copy(); bad[3] = -1
    refused(call(ref=bad))
    bad = query.copy(); bad[4] = nf
    refused(call(query=bad))
    bad = query.copy(); bad[2] = ref[2]
    refused(call(query=bad))                                       # ref == query
    for v in (np.nan, np.inf):
        bad = X.copy(); bad[100, 5] = v                            # a frame no closure names
        refused(call(X=bad))
        bad = Z.copy(); bad[6, 10] = v
        refused(call(Z=bad))
    bad = Z.copy(); bad[1, :9] *= 1.0 + 1e-5                       # R^T R - I = 2e-5
    refused(call(Z=bad))
    bad = Z.copy(); bad[1, :3] *= -1.0                             # a reflection
    refused(call(Z=bad))
    for kw in (dict(rot_tol=-1e-3), dict(rot_rate=np.nan), dict(trans_tol=np.inf), dict(trans_rate=-1.0), dict(n_seeds=0), dict(min_set=0),
               dict(min_set=-2)):
        refused(call(opts=L.ClosureOpts(**co.options(**kw))))
        with pytest.raises(L.LvbaError) as e:
            reg.closure_consistency(X, ref, query, Z, **kw)
        assert e.value.code == L.ERR_ARG and str(e.value), kw
    refused(lib.lvba_closure_consistency(0, 0, None, 0, None, None, None, C.byref(L.ClosureOpts(**co.options(n_seeds=0))), None, None, None,
                                         None, C.byref(n_keep)))
    # and the calls that are fine: NULL options are the defaults, n = 0 needs nothing but n_keep
    assert call() == L.OK and n_keep.value == want["n_keep"] and keep.astype(bool).tolist() == want["keep"]
    assert words.tobytes() == reg.closure_consistency(X, ref, query, Z)["words"].tobytes() and not rot.diagonal().any()
    n_keep.value = -5
    assert lib.lvba_closure_consistency(0, 0, None, 0, None, None, None, None, None, None, None, None, C.byref(n_keep)) == L.OK and n_keep.value == 0
    with pytest.raises(TypeError):
        reg.closure_consistency(X, ref, query, Z, radius=1.0)
    with pytest.raises(ValueError):
        reg.closure_consistency(X, ref[:-1], query, Z)


def test_consistent_closures_votes_out_the_fabricated_ones(pkg, pl):
    """§10e's twelve true closures and two fabricated ones as priors: exactly the twelve come back, in either orientation of a
    prior (a closure given as (query, ref, Z^-1) says the same and is tested the same)."""
    X, ref, query, Z = cc.two_lap_closures()
    P = pkg.Prior if hasattr(pkg, "Prior") else importlib.import_module("global-lvba_amd.balm").Prior
    priors = [P.relative(int(i), int(j), z, sigma_rot=0.01, sigma_pos=0.01) for i, j, z in zip(ref, query, Z)]
    kept, mask = pl.consistent_closures(X, priors)
    assert mask.tolist() == [True] * 12 + [False, False] and [id(p) for p in kept] == [id(p) for p in priors[:12]]
    flipped = [P.relative(int(j), int(i), co.inv(z), sigma_rot=0.01, sigma_pos=0.01) if k % 2 else p
               for k, (p, i, j, z) in enumerate(zip(priors, ref, query, Z))]
    kept, mask = pl.consistent_closures(X, flipped)
    assert mask.tolist() == [True] * 12 + [False, False] and [id(p) for p in kept] == [id(p) for p in flipped[:12]]
    assert pl.consistent_closures(X, []) [0] == [] and pl.consistent_closures(X, priors[:1])[1].tolist() == [False]
    assert pl.consistent_closures(X, priors[:1], min_set=1)[1].tolist() == [True]
    with pytest.raises(TypeError):
        pl.consistent_closures(X, priors, radius=2.0)


def strip(report):
    return [{k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in report]


def test_find_loop_closures_with_consistency(pkg, pl):
    """§10e's fixture at the drifted poses: with consistency=True the same closures are accepted as without, the twelve of lap B
    among them; the priors of lap B plus a measurement shifted by 2 m and a query tied to the wrong lap-A position come back as the
    twelve; consistency=None is the call without the keyword, key for key and byte for byte."""
    x = pc.drifted()
    shared = {k: pc.PLACE[k] for k in ("submap_size", "min_gap", "max_per_frame")}
    place = {k: v for k, v in pc.PLACE.items() if k not in shared}
    kw = dict(voxel_size=lc.VS, method="descriptor", place=place, **shared, **pc.ACCEPT, **pc.REG)
    with pkg.Scans(pc.clouds()) as sc:
        priors, report = pl.find_loop_closures(sc, x, **kw)
        priors_none, report_none = pl.find_loop_closures(sc, x, consistency=None, **kw)
        priors_on, report_on = pl.find_loop_closures(sc, x, consistency=True, **kw)
        priors_tight, report_tight = pl.find_loop_closures(sc, x, consistency=dict(min_set=1000), **kw)
        with pytest.raises(TypeError):
            pl.find_loop_closures(sc, x, consistency="yes", **kw)
        with pytest.raises(TypeError):
            pl.find_loop_closures(sc, x, consistency=dict(radius=1.0), **kw)
    assert strip(report_none) == strip(report) and all("consistent" not in r for r in report)
    assert [bytes(p) for p in priors_none] == [bytes(p) for p in priors]
    accepted = [(r["query"], r["submap"]) for r in report if r["accepted"]]
    lap_b = [r for r in report if r["accepted"] and r["query"] >= 12]
    print(f"{len(report)} candidates, {len(accepted)} accepted, {len(lap_b)} of them queries of lap B")
    assert len(lap_b) == 12
    assert [(r["query"], r["submap"]) for r in report_on if r["accepted"]] == accepted
    assert [bytes(p) for p in priors_on] == [bytes(p) for p in priors]
    assert all(r["consistent"] is (True if a["accepted"] else None) and r["reason"] == a["reason"] for r, a in zip(report_on, report))
    assert {k: v for k, v in strip(report_on)[0].items() if k != "consistent"} == strip(report)[0]
    # a min_set nobody meets: every accepted candidate is voted out and says why
    assert priors_tight == [] and all(r["consistent"] is (False if a["accepted"] else None) for r, a in zip(report_tight, report))
    assert all((r["accepted"], r["reason"]) == (False, "consistency") for r, a in zip(report_tight, report) if a["accepted"])
    assert all((r["accepted"], r["reason"]) == (False, a["reason"]) for r, a in zip(report_tight, report) if not a["accepted"])
    # the registered closures themselves, every pair of lap B's twelve: the largest rot / trans against the default tolerances
    P = pc.truth()
    mine = [p for p in priors if p.j >= 12]
    reg = importlib.import_module("global-lvba_amd.register")
    d = reg.closure_consistency(x, [p.i for p in mine], [p.j for p in mine], np.array([list(p.meas) for p in mine]), diagnostics=True)
    print(f"lap B's twelve: largest rot {d['rot'].max():.2e} rad, largest trans {d['trans'].max():.2e} m")
    assert d["adjacency"].all() and d["keep"].all()
    balm = importlib.import_module("global-lvba_amd.balm")
    moved = np.array(list(mine[3].meas)); moved[9:] += (2.0, 0.0, 0.0)
    wrong = co.mul(co.inv(P[8]), P[20])
    fake = [balm.Prior.relative(mine[3].i, mine[3].j, moved, sigma_rot=0.01, sigma_pos=0.01), balm.Prior.relative(2, 20, wrong, sigma_rot=0.01, sigma_pos=0.01)]
    kept, mask = pl.consistent_closures(x, mine + fake)
    assert mask.tolist() == [True] * 12 + [False, False] and [id(p) for p in kept] == [id(p) for p in mine]


def test_the_pose_fixture_keeps_its_four(pkg, pl):
    """§10d's fixture (drifted): the four candidates and their verdicts are those of the call without the check."""
    x = lc.drifted()
    kw = dict(submap_size=lc.S, voxel_size=lc.VS, radius=lc.RADIUS, min_gap=lc.MIN_GAP, **lc.ACCEPT, **lc.OPTS)
    with pkg.Scans([c[:, :3] for c in lc.scans()["clouds"]]) as sc:
        priors, report = pl.find_loop_closures(sc, x, **kw)
        priors_on, report_on = pl.find_loop_closures(sc, x, consistency=True, **kw)
    assert len(report) == 4 == len(report_on)
    assert [(r["accepted"], r["reason"]) for r in report_on] == [(r["accepted"], r["reason"]) for r in report]
    assert [bytes(p) for p in priors_on] == [bytes(p) for p in priors] and len(priors) >= 2
    assert [r["consistent"] for r in report_on] == [True if r["accepted"] else None for r in report]
