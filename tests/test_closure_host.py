"""CPU tests of the pairwise consistency of loop closures: the device header (csrc/closure_device.h) compiled for the host
against the numpy restatement (tests/closure_oracle.py), the conditions on the shared cases (tests/closure_cases.py, DESIGN.md
§10f), the argument checks of pipeline.consistent_closures and the struct layout."""
import ctypes
import importlib

import numpy as np
import pytest

from host_build import build_check

import closure_cases as cc
import closure_oracle as co

CASES = range(len(cc.cases()))
IDS = [c["name"] for c in cc.cases()]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("closure_check", tmp_path_factory.mktemp("emul_closure")))
    f64, i32, u64, u8 = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float64, np.int32, np.uint64, np.uint8))
    lib.emul_adjacency.argtypes = [f64, ctypes.c_int, i32, i32, f64, f64, u64, f64, f64]
    lib.emul_adjacency.restype = None
    lib.emul_set.argtypes = [ctypes.c_int, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32, i32, i32, i32, u64, u8]
    lib.emul_set.restype = ctypes.c_int32
    return lib


def host_adjacency(emul, c):
    M, o = len(c["Z"]), c["opts"]
    W = (M + 63) // 64
    adj, rot, trans = np.zeros((max(M, 1), max(W, 1)), np.uint64), np.zeros((max(M, 1), max(M, 1))), np.zeros((max(M, 1), max(M, 1)))
    pad = lambda a, t: np.ascontiguousarray(a, t) if M else np.zeros(12, t)
    emul.emul_adjacency(c["X"], M, pad(c["ref"], np.int32), pad(c["query"], np.int32), pad(c["Z"], np.float64),
                        np.array([o[t] for t in co.TOLS]), adj, rot, trans)
    return adj[:M, :W], rot[:M, :M], trans[:M, :M]


def host_set(emul, words, n_seeds, min_set, shortcut):
    M = len(words)
    W = (M + 63) // 64
    ns = min(n_seeds, M)
    deg, seeds, picks, n_picks = (np.zeros(max(k, 1), np.int32) for k in (M, ns, ns * M, ns))
    sets, keep = np.zeros((max(ns, 1), max(W, 1)), np.uint64), np.zeros(max(M, 1), np.uint8)
    n_keep = emul.emul_set(M, np.ascontiguousarray(words, np.uint64) if M else np.zeros(1, np.uint64), n_seeds, min_set, shortcut, deg, seeds,
                           picks, n_picks, sets, keep)
    return dict(deg=deg[:M].tolist(), seeds=seeds[:ns].tolist(), picks=[picks[k * M:k * M + n_picks[k]].tolist() for k in range(ns)],
                sets=co.rows_of(sets[:ns, :W]) if ns else [], keep=keep[:M].astype(bool).tolist(), n_keep=int(n_keep))


@pytest.mark.parametrize("k", CASES, ids=IDS)
def test_host_equals_the_oracle(emul, k):
    """Adjacency, degrees, seeds, every round's pick and the kept set are the oracle's; rot / trans within 1e-9 -- the project's own
    bar for decision margins, three orders below the 1e-6 the cases keep; the matrix is symmetric, its diagonal set, its padding
    zero; the early exit changes nothing."""
    c = cc.cases()[k]
    adj, g = cc.oracle(k)
    M, o = len(c["Z"]), c["opts"]
    words, rot, trans = host_adjacency(emul, c)
    err = max(np.abs(rot - adj["rot"]).max(initial=0.0), np.abs(trans - adj["trans"]).max(initial=0.0))
    print(f"{c['name']}: decision margin {adj['margin']:.2e}, largest |rot, trans - oracle| {err:.2e}, kept {g['n_keep']} of {M}, "
          f"rounds per seed {[len(p) for p in g['picks']][:8]}")
    assert adj["margin"] >= 1e-6
    assert words.tobytes() == co.words(adj["rows"], M).tobytes()
    assert err <= 1e-9
    rows = co.rows_of(words)
    assert all((rows[a] >> a) & 1 and rows[a] >> M == 0 for a in range(M))
    assert all(((rows[a] >> b) & 1) == ((rows[b] >> a) & 1) for a in range(M) for b in range(a))
    assert np.array_equal(rot, rot.T) and np.array_equal(trans, trans.T) and not rot.diagonal().any() and not trans.diagonal().any()
    plain = host_set(emul, words, o["n_seeds"], o["min_set"], 0)
    assert plain["deg"] == g["deg"] and plain["seeds"] == g["seeds"] and plain["picks"] == g["picks"] and plain["sets"] == g["sets"]
    assert plain["keep"] == g["keep"] and plain["n_keep"] == g["n_keep"]
    short = host_set(emul, words, o["n_seeds"], o["min_set"], 1)
    assert short["sets"] == g["sets"] and short["keep"] == g["keep"] and short["n_keep"] == g["n_keep"]
    assert all(s == p[:len(s)] for s, p in zip(short["picks"], g["picks"]))
    assert all(co.is_clique(adj["rows"], K) for K in g["sets"])


def test_set_search_on_random_graphs(emul):
    """The set search alone, on graphs no closure list of the cases gives: dense and sparse random graphs of 1 to 200 vertices,
    with many exact ties in degree and in a round's counts."""
    rng = np.random.default_rng(5)
    for M, p, n_seeds, min_set in [(1, 0.5, 3, 1), (7, 0.5, 7, 2), (24, 0.7, 4, 2), (64, 0.9, 32, 2), (65, 0.3, 65, 3), (129, 0.95, 8, 2),
                                   (200, 0.6, 1, 2), (200, 0.98, 32, 2)]:
        A = rng.random((M, M)) < p
        A = np.triu(A, 1)
        A = A | A.T | np.eye(M, dtype=bool)
        rows = [sum(1 << b for b in range(M) if A[a, b]) for a in range(M)]
        g = co.greedy(rows, n_seeds, min_set)
        for shortcut in (0, 1):
            h = host_set(emul, co.words(rows, M), n_seeds, min_set, shortcut)
            assert h["seeds"] == g["seeds"] and h["sets"] == g["sets"] and h["keep"] == g["keep"] and h["n_keep"] == g["n_keep"], (M, p)
            assert h["picks"] == g["picks"] if not shortcut else all(s == q[:len(s)] for s, q in zip(h["picks"], g["picks"]))
        assert all(co.is_clique(rows, K) for K in g["sets"])
        if M <= 24:
            assert co.popcount(max(g["sets"], key=co.popcount)) <= co.max_clique_size(rows)


def test_cases_meet_their_conditions():
    names = [c["name"] for c in cc.cases()]
    assert [len(cc.named(f"M = {M}")["Z"]) for M in (0, 1, 2, 63, 64, 65, 130)] == [0, 1, 2, 63, 64, 65, 130]
    by = {c["name"]: cc.oracle(k) for k, c in enumerate(cc.cases())}
    # sizes: nothing, a single closure below min_set, a pair, and group 0 whole at every size; 130 is three words with a ragged
    # last one and keeps more than a word's worth
    assert by["M = 0"][1]["n_keep"] == 0 and by["M = 1"][1]["n_keep"] == 0 and by["M = 2"][1]["keep"] == [True, True]
    for M in (63, 64, 65, 130):
        c = cc.named(f"M = {M}")
        assert by[c["name"]][1]["keep"] == [g == 0 for g in c["groups"]] and 0 < sum(g != 0 for g in c["groups"]) <= M // 9
    assert by["M = 130"][1]["n_keep"] == 117 > 64
    # the outlier groups are mutually consistent inside and with nobody outside
    c, (adj, _) = cc.named("M = 130"), by["M = 130"]
    D = co.dense(adj["rows"], 130)
    same = np.equal.outer(c["groups"], c["groups"])
    assert np.array_equal(D, same) and len(set(c["groups"])) == 6
    # the clauses, against the last closure
    adj, _ = by["clauses"]
    o = co.DEFAULTS
    D = co.dense(adj["rows"], 7)
    r, t, L = adj["rot"][6], adj["trans"][6], adj["L"][6]
    assert list(D[6]) == [True, False, True, False, True, True, True] and list(L) == [2, 4, 6, 8, 60, 70, 0]
    assert 0.8 * o["rot_tol"] < r[0] <= o["rot_tol"] and t[0] < 1e-9                                        # admitted, rotation binding
    assert r[1] > o["rot_tol"] + o["rot_rate"] * L[1] and t[1] < 1e-9                                       # rejected by rotation alone
    assert 0.7 * o["trans_tol"] < t[2] <= o["trans_tol"] and r[2] < 1e-9                                    # admitted, translation binding
    assert t[3] > o["trans_tol"] + o["trans_rate"] * L[3] and r[3] < 1e-9                                   # rejected by translation alone
    assert o["trans_tol"] < t[4] <= o["trans_tol"] + o["trans_rate"] * L[4] and abs(t[4] - t[3]) < 1e-9     # the rate term alone
    assert o["rot_tol"] < r[5] <= o["rot_tol"] + o["rot_rate"] * L[5] and abs(r[5] - r[1]) < 1e-9
    # the chain: a clique, not a connected component
    adj, g = by["chain"]
    assert co.dense(adj["rows"], 3).tolist() == [[True, True, False], [True, True, True], [False, True, True]]
    assert np.allclose(adj["trans"][0], [0, 0.12, 0.24], atol=1e-9) and g["seeds"] == [1, 0, 2] and g["picks"][0] == [0] and g["keep"] == [True, True, False]
    # two cliques of five: equal degrees everywhere, the first seed's set wins, and it is the one with the discrepancy
    c, (adj, g) = cc.named("two cliques"), by["two cliques"]
    assert g["deg"] == [4] * 10 and g["seeds"] == list(range(10)) and [co.popcount(K) for K in g["sets"]] == [5] * 10
    assert g["best"] == 0 and g["keep"] == [k % 2 == 0 for k in range(10)] and c["groups"][0] == 1
    assert g["picks"][0] == [2, 4, 6, 8]                                                                   # exact ties in a round: the lowest index
    # seeds and min_set
    one, many = by["n_seeds 1"][1], by["n_seeds > M"][1]
    assert len(one["seeds"]) == 1 and len(many["seeds"]) == 65 and one["keep"] == many["keep"] and one["n_keep"] == 59
    assert by["min_set above the best"][1]["n_keep"] == 0 and not any(by["min_set above the best"][1]["keep"])
    assert by["min_set met"][1]["n_keep"] == 12 == co.popcount(by["min_set above the best"][1]["sets"][0])
    # the lever arm: positions ~1 000 m, the cross-group angle is far below rot_tol and the translation above its bound
    c, (adj, g) = cc.named("lever arm"), by["lever arm"]
    assert np.abs(c["X"][:, 9:]).min() > 400 and np.linalg.norm(c["X"][:, 9:], axis=1).min() > 1400
    cross = ~np.equal.outer(c["groups"], c["groups"])
    assert adj["rot"][cross].max() < 0.2 * co.DEFAULTS["rot_tol"] and adj["trans"][cross].min() > 0.6
    assert not co.dense(adj["rows"], 18)[cross].any() and g["keep"] == [x == 0 for x in c["groups"]]
    # the two laps at the drifted poses: the twelve true closures, not the two fabricated ones
    adj, g = by["two laps, drifted"]
    assert g["keep"] == [True] * 12 + [False, False] and co.dense(adj["rows"], 14)[:12, :12].all() and not co.dense(adj["rows"], 14)[12:, :12].any()
    # greedy equals exact on every small case
    small = [n for n in names if len(cc.named(n)["Z"]) <= 24]
    assert len(small) >= 8
    for n in small:
        adj, g = by[n]
        if g["sets"]:
            assert max(co.popcount(K) for K in g["sets"]) == co.max_clique_size(adj["rows"]), n


def test_consistent_closures_refuses_what_it_cannot_check():
    pl = importlib.import_module("global-lvba_amd.pipeline")
    balm = importlib.import_module("global-lvba_amd.balm")
    X = cc.headed()
    T = co.IDENTITY
    off = co.rigid(t=(0.1, 0, 0))
    with pytest.raises(ValueError, match="not a relative prior"):
        pl.consistent_closures(X, [balm.Prior.pose(0, T, sigma_rot=1.0, sigma_pos=1.0)])
    with pytest.raises(ValueError, match="not a relative prior"):
        pl.consistent_closures(X, [balm.Prior.relative(0, 40, T, sigma_rot=1.0, sigma_pos=1.0), balm.Prior.position(3, [0, 0, 0], sigma=1.0)])
    with pytest.raises(ValueError, match="not a relative prior"):
        pl.consistent_closures(X, [(0, 40, T)])
    for kw in (dict(offset_i=off), dict(offset_j=off)):
        with pytest.raises(ValueError, match="offset"):
            pl.consistent_closures(X, [balm.Prior.relative(0, 40, T, sigma_rot=1.0, sigma_pos=1.0, **kw)])
    import inspect
    assert inspect.signature(pl.find_loop_closures).parameters["consistency"].default is None


def test_closure_struct_size_matches_the_header():
    L = importlib.import_module("global-lvba_amd._lib")
    # the layout of lvba_closure_opts against the header: tests/test_abi.py, every struct at once
    assert all(s in L.SYMBOLS for s in ("lvba_closure_default_opts", "lvba_closure_consistency"))


def test_registered_closures_of_the_two_laps_are_consistent():
    """§10e's twelve lap-B closures as the oracle registers them at the drifted poses (register_oracle, the priors by
    pipeline.registration_prior): all 66 pairs pass the default tolerances with room to spare, and the two fabricated closures of
    the GPU test contradict every one of them."""
    import place_cases as pc
    pl = importlib.import_module("global-lvba_amd.pipeline")
    x, P = pc.drifted(), pc.truth()
    cand = [c for c in pc.candidates()[0] if c[0] >= 12]
    assert len(cand) == 12
    ref, query, Z = [], [], []
    for q, w, r, s, _, _ in cand:
        _, o, (ok, _) = pc.oracle_register(q, w, r, s)
        assert ok
        p = pl.registration_prior(r, q, x[r], o["pose"], o["information"], o["rmse"], o["status"])
        ref.append(p.i); query.append(p.j); Z.append(list(p.meas))
    adj = co.adjacency(x, ref, query, np.array(Z))
    iu = np.triu_indices(12, 1)
    print(f"66 pairs: largest rot {adj['rot'][iu].max():.3e} rad, largest trans {adj['trans'][iu].max():.3e} m, margin {adj['margin']:.3e}")
    assert len(iu[0]) == 66 and co.dense(adj["rows"], 12).all() and adj["margin"] >= 1e-6
    assert adj["rot"].max() <= 0.5 * co.DEFAULTS["rot_tol"] and adj["trans"].max() <= 0.5 * co.DEFAULTS["trans_tol"]
    moved = np.array(Z[3]); moved[9:] += (2.0, 0.0, 0.0)
    ref += [ref[3], 2]; query += [query[3], 20]; Z += [list(moved), list(co.mul(co.inv(P[8]), P[20]))]
    adj = co.adjacency(x, ref, query, np.array(Z))
    g = co.greedy(adj["rows"])
    assert g["keep"] == [True] * 12 + [False, False] and not co.dense(adj["rows"], 14)[12:, :12].any() and adj["margin"] >= 1e-6
