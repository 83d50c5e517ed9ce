"""GPU tests of the descriptor matcher's depth-guided gate (lvba_match_set_depth, lvba_match_points, guided = 2; match.Matcher,
pipeline.match_image_pairs, run_full_pipeline(match_depth=True)) against the numpy restatement (tests/match_depth_oracle.py) on
the facade fixture (tests/match_depth_cases.py).  Every comparison is exact: the lifted points are multiplications
and additions of correctly rounded operands, and the fixture keeps every decision at least 1e-9 away from its bound
(test_match_depth_host.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import match_cases as mc
import match_depth_cases as mdc
import match_depth_oracle as mdo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(pkg):
    return importlib.import_module("global-lvba_amd.match")


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("global-lvba_amd.visual")


@pytest.fixture(scope="module")
def depth(V):
    with V.DepthImages.upload(mdc.facade()["depth"]) as d:
        yield d


def new_matcher(M, f, second=False):
    m = M.Matcher(f["descs"])
    m.set_geometry(f["keypoints"], f["intr"], f["Rcw2" if second else "Rcw"], f["tcw2" if second else "tcw"])
    return m


@pytest.fixture(scope="module")
def views(M, depth):
    with new_matcher(M, mdc.facade()) as m:
        m.set_depth(depth)
        yield m


def check_csr(got, want):
    matches, scores, off, count = got
    wm, ws, woff = want
    np.testing.assert_array_equal(off, woff)
    assert count == len(wm)
    np.testing.assert_array_equal(matches, wm)
    np.testing.assert_array_equal(scores, ws)


def same_bytes(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x[:3], y[:3])) and x[3] == y[3]


def refused(L, call):
    with pytest.raises(L.LvbaError) as e:
        call()
    assert e.value.code == L.ERR_ARG
    return e.value


def test_points_equal_the_oracle(views):
    geo = mdc.geometry()
    got, want = views.points(), np.concatenate(geo.points)
    assert got.shape == want.shape == (sum(mdc.COUNTS), 3)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert 0 < np.isnan(want[:, 0]).sum() < len(want)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("px", (8.0, 3.0))
def test_scan_equals_the_oracle(views, px):
    f, geo = mdc.facade(), mdc.geometry()
    for a, b in mdc.PAIRS:
        for x, y in ((int(a), int(b)), (int(b), int(a))):
            for got, want in zip(views.scan(x, y, guided=2, max_reproj_px=px), mdo.scan(f["descs"], x, y, geo, guided=2, max_reproj_px=px)):
                np.testing.assert_array_equal(got, want, err_msg=f"pair ({x}, {y})")


@pytest.mark.parametrize("kw", mdc.DEPTH_OPTION_SETS, ids=[str(i) for i in range(len(mdc.DEPTH_OPTION_SETS))])
def test_match_pairs_equals_the_oracle(views, kw):
    f, geo = mdc.facade(), mdc.geometry()
    got = views.match_pairs_csr(mdc.PAIRS, **kw)
    check_csr(got, mdo.match_pairs(f["descs"], mdc.PAIRS, geo, **kw))
    assert got[3] > 300
    assert same_bytes(got, views.match_pairs_csr(mdc.PAIRS, **kw))           # the same bytes on a second call


def test_the_other_modes_do_not_see_the_points(M, views):
    f = mdc.facade()
    with new_matcher(M, f) as bare:
        for kw in (dict(guided=0), dict(guided=1)):
            assert same_bytes(views.match_pairs_csr(mdc.PAIRS, **kw), bare.match_pairs_csr(mdc.PAIRS, **kw))
            for got, want in zip(views.scan(0, 1, **kw), bare.scan(0, 1, **kw)):
                assert got.tobytes() == want.tobytes()


def test_life_cycle(pkg, M, V, depth):
    L = pkg._lib
    f = mdc.facade()
    want1 = mdo.match_pairs(f["descs"], mdc.PAIRS, mdc.geometry(), guided=2)
    want2 = mdo.match_pairs(f["descs"], mdc.PAIRS, mdc.geometry(second=True), guided=2)
    with M.Matcher(f["descs"]) as m, V.DepthImages.upload(f["depth"][:3]) as three:
        refused(L, lambda: m.set_depth(depth))                                # no geometry yet
        assert not m.has_depth
        m.set_depth(None)                                                     # dropping nothing is fine
        m.set_geometry(f["keypoints"], f["intr"], f["Rcw"], f["tcw"])
        refused(L, lambda: m.match_pairs_csr(mdc.PAIRS, guided=2))            # geometry, but no points
        assert b"lvba_match_set_depth" in m.lib.lvba_last_error()
        refused(L, lambda: m.scan(0, 1, guided=2))
        refused(L, lambda: m.points())
        refused(L, lambda: m.set_depth(three))                                # a depth set of another image count
        assert not m.has_depth
        m.set_depth(depth)
        assert m.has_depth
        first = m.match_pairs_csr(mdc.PAIRS, guided=2)
        check_csr(first, want1)
        pts = m.points()
        refused(L, lambda: m.set_depth(three))                                # refused: the old points and results stay
        assert m.has_depth and m.points().tobytes() == pts.tobytes()
        assert same_bytes(first, m.match_pairs_csr(mdc.PAIRS, guided=2))
        R = f["Rcw"].copy(); R[2, 0, 0] = np.nan
        refused(L, lambda: m.set_geometry(f["keypoints"], f["intr"], R, f["tcw"]))   # a refused set_geometry keeps them too
        assert m.has_depth and same_bytes(first, m.match_pairs_csr(mdc.PAIRS, guided=2))
        m.set_geometry(f["keypoints"], f["intr"], f["Rcw2"], f["tcw2"])       # new poses: the points went with the old ones
        assert not m.has_depth
        refused(L, lambda: m.match_pairs_csr(mdc.PAIRS, guided=2))
        assert b"lvba_match_set_depth" in m.lib.lvba_last_error()
        m.set_depth(depth)
        second = m.match_pairs_csr(mdc.PAIRS, guided=2)
        check_csr(second, want2)
        np.testing.assert_array_equal(m.points(), np.concatenate(mdc.geometry(second=True).points))
        assert not same_bytes(first, second)
        m.set_depth(None)
        assert not m.has_depth
        refused(L, lambda: m.match_pairs_csr(mdc.PAIRS, guided=2))
        refused(L, lambda: m.points())
        check_csr(m.match_pairs_csr(mdc.PAIRS, guided=1), mdo.match_pairs(f["descs"], mdc.PAIRS, mdc.geometry(second=True), guided=1))


def test_refused_calls_write_nothing(pkg, M, views):
    L = pkg._lib
    lib = views.lib
    f = mdc.facade()
    pairs = np.ascontiguousarray(mdc.PAIRS[:3], np.int32)

    def pairs_call(m, opts):
        matches, scores = np.full((16, 2), -7, np.int32), np.full(16, -7, np.int32)
        o, cnt = np.full(len(pairs) + 2, -7, np.int64), C.c_int64(-7)
        rc = lib.lvba_match_pairs(m._h, len(pairs), pairs.ctypes.data, C.byref(opts), 16, matches.ctypes.data, scores.ctypes.data,
                                  o.ctypes.data, C.byref(cnt))
        assert (matches == -7).all() and (scores == -7).all() and (o == -7).all() and cnt.value == -7
        return rc

    def scan_call(m, opts):
        out = np.full((3, 400), -7, np.int32)
        rc = lib.lvba_match_scan(m._h, 0, 1, C.byref(opts), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
        assert (out == -7).all()
        return rc

    for bad in (dict(guided=3), dict(guided=2, max_reproj_px=0.0), dict(max_reproj_px=np.nan), dict(max_reproj_px=np.inf),
                dict(guided=2, max_reproj_px=-1.0)):
        assert pairs_call(views, M.match_opts(**bad)) == L.ERR_ARG, bad
        assert scan_call(views, M.match_opts(**bad)) == L.ERR_ARG, bad
    with new_matcher(M, f) as bare:                                           # geometry, no points
        assert pairs_call(bare, M.match_opts(guided=2)) == L.ERR_ARG
        assert b"lvba_match_set_depth" in lib.lvba_last_error()
        assert scan_call(bare, M.match_opts(guided=2)) == L.ERR_ARG
        world = np.full((sum(mdc.COUNTS), 3), -7.0)
        assert lib.lvba_match_points(bare._h, world.ctypes.data) == L.ERR_ARG and (world == -7.0).all()
        assert lib.lvba_match_set_depth(None, None) == L.ERR_ARG
    assert lib.lvba_match_points(views._h, None) == L.ERR_ARG
    assert M.match_opts().max_reproj_px == 8.0 and C.sizeof(L.MatchOpts) == 40


def test_matches_feed_build_tracks(pkg, V):
    """pipeline.match_image_pairs(depth=...) -> the track builder on the four views: every track is one 3-D point, and the textures
    repeated along the baseline of views 0-2 are among the tracks."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    f, geo = mdc.facade(), mdc.geometry()
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    descs, kps = f["descs"][:4], f["keypoints"][:4]
    with V.DepthImages.upload(f["depth"][:4]) as d4:
        matches = pl.match_image_pairs(descs, pairs, keypoints=kps, Rcw=f["Rcw"][:4], tcw=f["tcw"][:4], intr=f["intr"], depth=d4)
        epipolar = pl.match_image_pairs(descs, pairs, keypoints=kps, Rcw=f["Rcw"][:4], tcw=f["tcw"][:4], intr=f["intr"])
    for (a, b), got in zip(pairs, matches):
        np.testing.assert_array_equal(got, mdo.match_pair(f["descs"], a, b, geo, guided=2)[0])

    def tracks_of(ms):
        off, img, kp = pl.build_components([len(x) for x in descs], pairs, ms, obser_thr=3)
        return [{int(f["point"][i][k]) for i, k in zip(img[off[t]:off[t + 1]], kp[off[t]:off[t + 1]])} for t in range(len(off) - 1)]

    tracks = tracks_of(matches)
    assert all(len(t) == 1 and -1 not in t for t in tracks)
    found = {next(iter(t)) for t in tracks}
    assert set(range(mdc.N_REP)) <= found                                    # every repeated point is seen by views 0, 1 and 2
    # under the epipolar gate the baseline pairs give none of them; what is left comes through view 3 alone
    assert len({p for t in tracks_of(epipolar) for p in t if 0 <= p < mdc.N_REP}) < mdc.N_REP


def test_full_pipeline_with_match_depth(pkg, monkeypatch):
    """run_full_pipeline(match_fn=..., match_depth=True) on the small sequence of the pipeline tests: the matcher gets the depth
    images of the visual stage, rendered once at the LiDAR-refined poses, and the visual stage runs on its matches."""
    import test_gpu_pipeline as tp
    pl = importlib.import_module("global-lvba_amd.pipeline")
    vis = importlib.import_module("global-lvba_amd.visual")
    d = tp._dataset(n_frames=10, pts=20000, n_land=300, seed=64)
    rng = np.random.default_rng(64)
    tex = mc.sift_like(rng, len(d["X"]))
    descs = [mc.noisy(rng, tex[np.asarray(ids, np.int64)], 6) if len(ids) else np.zeros((0, 128), np.uint8) for ids in d["lm_of"]]
    seen, renders = [], []
    render = vis.DepthImages.render

    def match_fn(cam_poses, depth=None):
        seen.append((depth.n_images, depth.width, depth.height))
        Rcw, tcw = pl.camera_from_imu(cam_poses, tp.RCB, tp.TCI)
        return d["pairs"], pl.match_image_pairs(descs, d["pairs"], keypoints=d["kps"], Rcw=Rcw, tcw=tcw, intr=tp.INTR, depth=depth)

    def counting_render(*a, **k):
        renders.append(1)
        return render(*a, **k)

    monkeypatch.setattr(vis.DepthImages, "render", counting_render)
    out = pl.run_full_pipeline(d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"],
                               [], [], match_fn=match_fn, match_depth=True, window_size=5, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5),
                               stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    assert seen == [(len(d["img_t"]), tp.W, tp.H)] and len(renders) == 1      # rendered once, shared with the visual stage
    assert out["pairs"] is d["pairs"] and len(out["matches"]) == len(d["pairs"])
    assert sum(len(m) for m in out["matches"]) > 0
    v = out["visual"]
    assert v["n_components"] > 0 and "termination" in v
