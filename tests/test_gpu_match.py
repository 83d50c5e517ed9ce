"""GPU tests of the descriptor matcher (lvba_match_*, match.Matcher, pipeline.match_image_pairs) against the numpy restatement
(tests/match_oracle.py) on the shared fixtures (tests/match_cases.py).  Scores, columns and matches are integers:
every comparison is exact.  The fixtures keep every fp64 decision at least 1e-9 away from its bound (test_match_host.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import match_cases as mc
import match_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(pkg):
    return importlib.import_module("global-lvba_amd.match")


@pytest.fixture(scope="module")
def plain(M):
    with M.Matcher(mc.unguided()["descs"]) as m:
        yield m


@pytest.fixture(scope="module")
def views(M):
    g = mc.guided()
    with M.Matcher(g["descs"]) as m:
        m.set_geometry(g["keypoints"], g["intr"], g["Rcw"], g["tcw"])
        yield m


def check_csr(got, want):
    matches, scores, off, count = got
    wm, ws, woff = want
    np.testing.assert_array_equal(off, woff)
    assert count == len(wm)
    np.testing.assert_array_equal(matches, wm)
    np.testing.assert_array_equal(scores, ws)


def test_scan_equals_the_oracle(plain):
    u = mc.unguided()
    for a, b in u["pairs"]:
        for x, y in ((int(a), int(b)), (int(b), int(a))):
            for got, want in zip(plain.scan(x, y), mo.scan(u["descs"], x, y)):
                np.testing.assert_array_equal(got, want, err_msg=f"pair ({x}, {y})")


def test_scan_of_a_large_image(M):
    """32 768 descriptors in one image (256 workgroups of rows one way, 1024 column tiles the other) against fp64 BLAS scores,
    which are exact for integers of this size"""
    rng = np.random.default_rng(9)
    big, small = mc.sift_like(rng, 32768), mc.sift_like(rng, 257)
    big[1000:1200] = mc.noisy(rng, small[:200], 10)
    S = (big.astype(np.float64) @ small.astype(np.float64).T).astype(np.int64)
    with M.Matcher([big, small]) as m:
        for got, want in zip(m.scan(0, 1), mo.top_two(S)):
            np.testing.assert_array_equal(got, want)
        for got, want in zip(m.scan(1, 0), mo.top_two(S.T)):
            np.testing.assert_array_equal(got, want)
        got = m.match_pairs([(1, 0)])[0]
    assert len(got) >= 190 and all(c == 1000 + r for r, c in got)


@pytest.mark.parametrize("kw", mc.OPTION_SETS, ids=[str(i) for i in range(len(mc.OPTION_SETS))])
def test_match_pairs_equals_the_oracle(plain, kw):
    u = mc.unguided()
    got = plain.match_pairs_csr(u["pairs"], **kw)
    check_csr(got, mo.match_pairs(u["descs"], u["pairs"], **kw))
    again = plain.match_pairs_csr(u["pairs"], **kw)                       # the same bytes on a second call
    for x, y in zip(got[:3], again[:3]):
        assert x.tobytes() == y.tobytes()


def test_pair_order_and_transposition(plain):
    u = mc.unguided()
    blocks = plain.match_pairs(u["pairs"])
    perm = np.random.default_rng(1).permutation(len(u["pairs"]))
    shuffled = plain.match_pairs(u["pairs"][perm])                        # each pair's block unchanged wherever it stands
    for k, p in enumerate(perm):
        np.testing.assert_array_equal(shuffled[k], blocks[p])
    # (b, a): sorted by its own row and the oracle's list.  It is the transposed list of (a, b) wherever the ratio clause passes on
    # both sides: the distance and the mutual clause are symmetric, the ratio clause looks at the second best of its own row.
    swapped = plain.match_pairs(u["pairs"][:, ::-1])
    exact = 0
    for k, (a, b) in enumerate(u["pairs"]):
        a, b = int(a), int(b)
        np.testing.assert_array_equal(swapped[k], mo.match_pair(u["descs"], b, a)[0])
        assert (np.diff(swapped[k][:, 0]) > 0).all()
        fwd, bwd = set(map(tuple, blocks[k].tolist())), set((r, c) for c, r in swapped[k].tolist())
        best, s1, s2 = mo.scan(u["descs"], a, b)
        back, t1, t2 = mo.scan(u["descs"], b, a)
        sym = {(r, int(c)) for r, c in enumerate(best) if c >= 0 and back[c] == r and mo.distance(s1[r]) < 0.7}
        ratio_a = {r for r in range(len(best)) if mo.distance(s1[r]) < 0.8 * mo.distance(s2[r])}
        ratio_b = {c for c in range(len(back)) if mo.distance(t1[c]) < 0.8 * mo.distance(t2[c])}
        assert fwd | bwd <= sym and fwd & bwd == {(r, c) for r, c in sym if r in ratio_a and c in ratio_b}
        exact += fwd == bwd
    assert exact >= len(u["pairs"]) // 2
    assert sum(len(b) for b in blocks) > 500 and any(len(b) == 0 for b in blocks)
    one_sided = plain.match_pairs(u["pairs"], mutual=0)                   # the oracle's one-sided list
    for (a, b), got in zip(u["pairs"], one_sided):
        np.testing.assert_array_equal(got, mo.match_pair(u["descs"], int(a), int(b), mutual=0)[0])
    matches, scores, off, count = plain.match_pairs_csr(np.zeros((0, 2), np.int32))   # an empty pair list
    assert count == 0 and off.tolist() == [0] and len(matches) == 0


@pytest.mark.parametrize("kw", mc.GUIDED_OPTION_SETS, ids=[str(i) for i in range(len(mc.GUIDED_OPTION_SETS))])
def test_guided_equals_the_oracle(views, kw):
    g, geo = mc.guided(), mc.guided_geometry()
    for a, b in g["pairs"]:
        for x, y in ((int(a), int(b)), (int(b), int(a))):
            for got, want in zip(views.scan(x, y, **kw), mo.scan(g["descs"], x, y, geo, **kw)):
                np.testing.assert_array_equal(got, want, err_msg=f"pair ({x}, {y})")
    check_csr(views.match_pairs_csr(g["pairs"], **kw), mo.match_pairs(g["descs"], g["pairs"], geo, **kw))
    check_csr(views.match_pairs_csr(g["pairs"]), mo.match_pairs(g["descs"], g["pairs"]))      # unguided stays available


def test_set_geometry_again_changes_the_result_as_the_oracle_says(M):
    g = mc.guided()
    with M.Matcher(g["descs"]) as m:
        m.set_geometry(g["keypoints"], g["intr"], g["Rcw"], g["tcw"])
        first = m.match_pairs_csr(g["pairs"], guided=1)
        m.set_geometry(g["keypoints"], g["intr"], g["Rcw2"], g["tcw2"])
        second = m.match_pairs_csr(g["pairs"], guided=1)
    check_csr(first, mo.match_pairs(g["descs"], g["pairs"], mc.guided_geometry(), guided=1))
    check_csr(second, mo.match_pairs(g["descs"], g["pairs"], mc.guided_geometry(second=True), guided=1))
    assert first[3] != second[3]


def test_capacity(plain):
    u = mc.unguided()
    wm, ws, woff = mo.match_pairs(u["descs"], u["pairs"])
    cap = 100
    pairs = np.ascontiguousarray(u["pairs"], np.int32)
    matches = np.full((cap + 8, 2), -7, np.int32)
    scores = np.full(cap + 8, -7, np.int32)
    off = np.zeros(len(pairs) + 1, np.int64)
    count = C.c_int64(-1)
    rc = plain.lib.lvba_match_pairs(plain._h, len(pairs), pairs.ctypes.data, None, cap, matches.ctypes.data, scores.ctypes.data,
                                    off.ctypes.data, C.byref(count))
    assert rc == 0 and count.value == len(wm) > cap
    np.testing.assert_array_equal(off, woff)                              # the full match_off
    np.testing.assert_array_equal(matches[:cap], wm[:cap]); np.testing.assert_array_equal(scores[:cap], ws[:cap])
    assert (matches[cap:] == -7).all() and (scores[cap:] == -7).all()    # exactly `capacity` rows
    rc = plain.lib.lvba_match_pairs(plain._h, len(pairs), pairs.ctypes.data, None, 0, None, None, off.ctypes.data, C.byref(count))
    assert rc == 0 and count.value == len(wm)                             # counting alone; scores may be NULL


def test_refused_calls_write_nothing(pkg, M, plain):
    L = pkg._lib
    lib = plain.lib
    u, g = mc.unguided(), mc.guided()
    n_img = plain.n_images

    def pairs_call(m, pairs, opts=None, n_pairs=None, count=True, off=True, cap=16):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        matches, scores = np.full((16, 2), -7, np.int32), np.full(16, -7, np.int32)
        o, cnt = np.full(len(pairs) + 2, -7, np.int64), C.c_int64(-7)
        rc = lib.lvba_match_pairs(m._h, len(pairs) if n_pairs is None else n_pairs, pairs.ctypes.data, C.byref(opts) if opts else None, cap,
                                  matches.ctypes.data, scores.ctypes.data, o.ctypes.data if off else None, C.byref(cnt) if count else None)
        assert (matches == -7).all() and (scores == -7).all() and (o == -7).all() and cnt.value == -7
        return rc

    assert pairs_call(plain, [(2, 4)], count=False) == L.ERR_ARG                     # null required pointers
    assert pairs_call(plain, [(2, 4)], off=False) == L.ERR_ARG
    assert pairs_call(plain, [(2, 4)], n_pairs=-1) == L.ERR_ARG                      # negative counts
    assert pairs_call(plain, [(2, 4)], cap=-1) == L.ERR_ARG
    assert pairs_call(plain, [(2, 4), (2, n_img)]) == L.ERR_ARG                      # a pair outside the images
    assert pairs_call(plain, [(-1, 4)]) == L.ERR_ARG
    assert pairs_call(plain, [(2, 4), (3, 3)]) == L.ERR_ARG                          # a == b
    for bad in (dict(max_distance=0.0), dict(max_distance=np.nan), dict(max_distance=np.inf), dict(max_ratio=0.0), dict(max_ratio=1.5),
                dict(max_ratio=np.nan), dict(mutual=2), dict(guided=-1), dict(guided=1, max_epipolar_px=0.0),
                dict(max_epipolar_px=np.nan), dict(max_epipolar_px=np.inf)):
        assert pairs_call(plain, [(2, 4)], M.match_opts(**bad)) == L.ERR_ARG, bad
    assert pairs_call(plain, [(2, 4)], M.match_opts(guided=1)) == L.ERR_ARG         # guided without geometry
    assert b"set_geometry" in lib.lvba_last_error()
    best = np.full(40, -7, np.int32)
    o = M.match_opts(guided=1)
    assert lib.lvba_match_scan(plain._h, 2, 4, C.byref(o), best.ctypes.data, best.ctypes.data, best.ctypes.data) == L.ERR_ARG
    assert lib.lvba_match_scan(plain._h, 2, 2, None, best.ctypes.data, best.ctypes.data, best.ctypes.data) == L.ERR_ARG
    assert lib.lvba_match_scan(plain._h, 2, 4, None, None, best.ctypes.data, best.ctypes.data) == L.ERR_ARG
    assert (best == -7).all()

    h = C.c_void_p()
    d = u["descs"][2]

    def create(off):
        off = np.asarray(off, np.int64)
        return lib.lvba_match_create(0, len(off) - 1, off.ctypes.data, d.ctypes.data, C.byref(h))

    assert create([0, 20, 10]) == L.ERR_ARG and not h.value                          # desc_off goes down
    assert create([1, 20]) == L.ERR_ARG and not h.value
    assert create([0, (1 << 20) + 1]) == L.ERR_ARG and not h.value                   # above the per-image limit (checked before any read)
    assert lib.lvba_match_create(0, -1, np.zeros(1, np.int64).ctypes.data, d.ctypes.data, C.byref(h)) == L.ERR_ARG
    assert lib.lvba_match_create(0, 1, None, d.ctypes.data, C.byref(h)) == L.ERR_ARG
    assert lib.lvba_match_create(0, 1, np.array([0, 31], np.int64).ctypes.data, d.ctypes.data, None) == L.ERR_ARG

    with M.Matcher(g["descs"]) as m:                                                 # geometry that is refused keeps what was there
        def geometry(intr=g["intr"], R=g["Rcw"], t=g["tcw"]):
            try:
                m.set_geometry(g["keypoints"], intr, R, t)
            except L.LvbaError as e:
                return e.code
            return 0
        assert geometry() == 0
        want = m.match_pairs_csr(g["pairs"], guided=1)
        R = g["Rcw"].copy(); R[2, 0, 0] = np.nan
        assert geometry(R=R) == L.ERR_ARG                                            # non-finite geometry
        t = g["tcw"].copy(); t[1, 2] = np.inf
        assert geometry(t=t) == L.ERR_ARG
        intr = g["intr"].copy(); intr[4] = np.nan
        assert geometry(intr=intr) == L.ERR_ARG
        R = g["Rcw"].copy(); R[3] = R[3] * (1 + 1e-5)
        assert geometry(R=R) == L.ERR_ARG                                            # not orthonormal within 1e-6
        R = g["Rcw"].copy(); R[3] = R[3] * (1 + 1e-8)
        assert geometry(R=R) == 0 and geometry() == 0                                # within: accepted
        got = m.match_pairs_csr(g["pairs"], guided=1)
        for x, y in zip(got[:3], want[:3]):
            assert x.tobytes() == y.tobytes()


def test_matches_feed_build_tracks(pkg):
    """pipeline.match_image_pairs -> the track builder on the four views: every track is one 3-D point, and the points seen in all
    four views come out, the repeated textures among them."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    g, geo = mc.guided(), mc.guided_geometry()
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    descs, kps = g["descs"][:4], g["keypoints"][:4]
    matches = pl.match_image_pairs(descs, pairs, keypoints=kps, Rcw=g["Rcw"][:4], tcw=g["tcw"][:4], intr=g["intr"])
    assert len(matches) == len(pairs)
    g4 = mo.Geometry(kps, g["intr"], g["Rcw"][:4], g["tcw"][:4])
    for (a, b), got in zip(pairs, matches):
        np.testing.assert_array_equal(got, mo.match_pair(descs, a, b, g4, guided=1)[0])
    off, img, kp = pl.build_components([len(d) for d in descs], pairs, matches, obser_thr=3)
    tracks = [{int(g["point"][i][k]) for i, k in zip(img[off[t]:off[t + 1]], kp[off[t]:off[t + 1]])} for t in range(len(off) - 1)]
    assert all(len(t) == 1 and -1 not in t for t in tracks)
    found = {next(iter(t)) for t in tracks}
    in_all = set.intersection(*({int(p) for p in g["point"][v] if p >= 0} for v in range(4)))
    assert len(in_all) >= 100 and len(found & in_all) >= 0.9 * len(in_all)
    assert len({p for p in found if p < g["n_repeated"]}) >= 40
    unguided = pl.match_image_pairs(descs, pairs)                                   # without geometry: pairs kept, possibly empty
    assert len(unguided) == len(pairs)
    off_u, img_u, kp_u = pl.build_components([len(d) for d in descs], pairs, unguided, obser_thr=3)
    assert not {int(g["point"][i][k]) for i, k in zip(img_u, kp_u)} & set(range(g["n_repeated"]))
