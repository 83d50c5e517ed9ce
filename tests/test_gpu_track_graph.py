"""GPU tests of the device track builder (lvba_trackgraph_*; trackgraph.TrackGraph, pipeline.build_components_device,
build_tracks_and_fuse(device_tracks=True), run_full_pipeline(device_tracks=True)) against the host mirror -- pipeline.match_graph /
match_components / bfs_order, which tests/test_ref_system.py pins to the reference -- on the cases of tests/track_graph_cases.py
(DESIGN.md §10j).  Every output is a discrete structure with one right answer: every comparison is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import track_graph_cases as tc
from test_track_graph_host import fuse_stubs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def TG(pkg):
    return importlib.import_module("global-lvba_amd.trackgraph")


def make(TG, name, thr, uv=True):
    c = tc.case(name)
    return TG.TrackGraph(c["keypoints"] if uv else c["n_keypoints"], c["pairs"], c["matches"], obser_thr=thr)


def uv_of(name, img, kp):
    c = tc.case(name)
    flat = np.concatenate(c["keypoints"]) if c["keypoints"] else np.zeros((0, 2), np.float32)
    kp_off = np.concatenate([[0], np.cumsum(c["n_keypoints"])]).astype(np.int64)
    return flat[kp_off[img] + kp]


def check_orders(got, name, thr, attempt, comp=None):
    for x, y in zip(got[:3], tc.expected_orders(name, thr, attempt, comp)):
        np.testing.assert_array_equal(x, y, err_msg=f"{name} {thr} attempt {attempt}")
    if len(got) == 4:
        assert got[3].dtype == np.float32 and got[3].tobytes() == uv_of(name, got[1], got[2]).tobytes()


@pytest.mark.parametrize("name", tc.NAMES)
def test_info_components_and_first_orders(TG, name):
    for thr in tc.THRESHOLDS:
        want = tc.expected(name, thr)
        with make(TG, name, thr) as g:
            info = dict(g.info)
            rounds = info.pop("cc_rounds")
            assert info == want["info"], (name, thr)
            assert 0 <= rounds <= 64 and (rounds >= 1) == (want["info"]["n_edges"] > 0)
            off, img, kp, images = g.components()
            for x, key in ((off, "comp_off"), (img, "mem_img"), (kp, "mem_kp"), (images, "comp_images")):
                np.testing.assert_array_equal(x, want[key], err_msg=f"{name} {thr} {key}")
            check_orders(g.orders(uv=bool(tc.case(name)["keypoints"])), name, thr, 0)
            check_orders(g.orders(), name, thr, 0)


@pytest.mark.parametrize("name,thresholds", [("random", tc.THRESHOLDS), ("thresholds", tc.THRESHOLDS), ("hub", (3,))])
def test_every_attempt_of_every_component(TG, name, thresholds):
    """the retry loop's later attempts: the BFS from every member of every component"""
    for thr in thresholds:
        with make(TG, name, thr) as g:
            for a in tc.attempts_of(name, thr):
                comp = tc.with_more_than(name, thr, a)
                check_orders(g.orders(comp, a, uv=True), name, thr, a, comp)


def test_chain_from_both_ends_and_the_middle(TG):
    with make(TG, "chain", 3) as g:
        assert g.info["n_components"] == 1 and g.info["largest_component"] == 300
        for a in tc.CHAIN_ATTEMPTS:
            check_orders(g.orders(None, a, uv=True), "chain", 3, a)


@pytest.mark.parametrize("name", ("giant", "four_views"))
def test_subsets_of_the_components(TG, name):
    with make(TG, name, 3) as g:
        n = g.info["n_components"]
        assert n > 3
        third = list(range(0, n, 3))
        check_orders(g.orders(third, 0, uv=True), name, 3, 0, third)
        check_orders(g.orders(third, 1, uv=True), name, 3, 1, third)
        for one in ([0], [n - 1], [n // 2]):
            check_orders(g.orders(one, 2, uv=True), name, 3, 2, one)
        assert [len(x) for x in g.orders([], 0, uv=True)] == [1, 0, 0, 0]


def test_device_components_equal_build_components(pkg):
    pl = tc.pipeline()
    for name in ("four_views", "random", "giant", "no_pairs"):
        c = tc.case(name)
        for x, y in zip(pl.build_components_device(c["n_keypoints"], c["pairs"], c["matches"], 3),
                        pl.build_components(c["n_keypoints"], c["pairs"], c["matches"], 3)):
            np.testing.assert_array_equal(x, y)
            assert x.dtype == y.dtype


def test_same_bytes_on_a_second_call_and_a_second_graph(TG):
    """the epoch is reused without stale marks (the same components walked again, from the same and from other members), and the
    atomics of the label rounds leave no trace in the outputs"""
    for name in ("hub", "giant", "random"):
        with make(TG, name, 3) as g, make(TG, name, 3) as h:
            first = g.orders(uv=True)
            g.orders(None, 1)
            again = g.orders(uv=True)
            other = h.orders(uv=True)
            for x, y, z in zip(first, again, other):
                assert x.tobytes() == y.tobytes() == z.tobytes()
            for x, y in zip(g.components(), h.components()):
                assert x.tobytes() == y.tobytes()
            a, b = dict(g.info), dict(h.info)
            a.pop("cc_rounds"); b.pop("cc_rounds")
            assert a == b


def test_refusals_write_nothing(pkg, TG):
    L = pkg._lib
    lib = L.load()
    c = tc.case("thresholds")
    kp_off = np.concatenate([[0], np.cumsum(c["n_keypoints"])]).astype(np.int64)
    pairs = np.asarray(c["pairs"], np.int32)
    match_off = np.concatenate([[0], np.cumsum([len(m) for m in c["matches"]])]).astype(np.int64)
    matches = np.ascontiguousarray(np.concatenate(c["matches"]), np.int32)
    uv = np.ascontiguousarray(np.concatenate(c["keypoints"]), np.float32)
    M, P = len(c["n_keypoints"]), len(pairs)

    def create(M=M, kp_off=kp_off, uv=uv, P=P, pairs=pairs, match_off=match_off, matches=matches, thr=3, out=True):
        h, info = C.c_void_p(0x5a5a), L.TrackGraphInfo()
        C.memset(C.byref(info), 0x5a, C.sizeof(info))
        p = lambda a: None if a is None else a.ctypes.data
        rc = lib.lvba_trackgraph_create(0, M, p(kp_off), p(uv), P, p(pairs), p(match_off), p(matches), thr, C.byref(h) if out else None, C.byref(info))
        assert h.value == 0x5a5a and bytes(info) == b"\x5a" * C.sizeof(info)
        return rc

    assert create(out=False) == L.ERR_ARG and create(kp_off=None) == L.ERR_ARG and create(pairs=None) == L.ERR_ARG
    assert create(match_off=None) == L.ERR_ARG and create(matches=None) == L.ERR_ARG
    assert create(M=-1) == L.ERR_ARG and create(P=-1) == L.ERR_ARG
    for thr in (0, -3):
        assert create(thr=thr) == L.ERR_ARG
    bad = kp_off.copy(); bad[0] = 1
    assert create(kp_off=bad) == L.ERR_ARG
    bad = kp_off.copy(); bad[2] = bad[1] - 1
    assert create(kp_off=bad) == L.ERR_ARG
    bad = match_off.copy(); bad[0] = 1
    assert create(match_off=bad) == L.ERR_ARG
    bad = match_off.copy(); bad[1], bad[2] = bad[2], bad[1] - 1
    assert create(match_off=bad) == L.ERR_ARG
    for a, b in ((0, M), (-1, 1), (2, 2)):
        bad = pairs.copy(); bad[1] = (a, b)
        assert create(pairs=bad) == L.ERR_ARG
    # the two 32-bit limits, checked before anything behind the offsets is read: there is nothing behind them
    assert create(M=2, kp_off=np.array([0, 5, 2 ** 31], np.int64), uv=None, P=0) == L.ERR_UNSUPPORTED
    assert create(M=2, kp_off=np.array([0, 5, 2 ** 31 - 1], np.int64), uv=None, P=1, pairs=np.array([[0, 1]], np.int32),
                  match_off=np.array([0, 2 ** 30], np.int64), matches=None) == L.ERR_UNSUPPORTED

    with make(TG, "thresholds", 3) as g, make(TG, "thresholds", 3, uv=False) as bare:
        comp_off = g.components()[0]
        n, total = g.info["n_components"], int(comp_off[-1])
        sizes = np.diff(comp_off)
        assert n >= 3 and sizes.min() < sizes.max()

        def orders(h=g, n=n, comp=None, attempt=0, off=True, img=True, kp=True, want_uv=True):
            o, i, k, u = np.full(n + 1 if n >= 0 else 1, -7, np.int64), np.full(total, -7, np.int32), np.full(total, -7, np.int32), np.full((total, 2), -7, np.float32)
            sel = None if comp is None else np.asarray(comp, np.int64)
            rc = lib.lvba_trackgraph_orders(h._h if h is not None else None, n, None if sel is None else sel.ctypes.data, attempt,
                                            o.ctypes.data if off else None, i.ctypes.data if img else None, k.ctypes.data if kp else None,
                                            u.ctypes.data if want_uv else None)
            assert (o == -7).all() and (i == -7).all() and (k == -7).all() and (u == -7).all()
            return rc

        assert orders(h=None) == L.ERR_ARG and orders(off=False) == L.ERR_ARG and orders(img=False) == L.ERR_ARG and orders(kp=False) == L.ERR_ARG
        assert orders(n=-1) == L.ERR_ARG and orders(n=n - 1) == L.ERR_ARG                 # comp = NULL asks for all of them
        assert orders(attempt=-1) == L.ERR_ARG and orders(attempt=int(sizes.min())) == L.ERR_ARG
        assert orders(n=2, comp=[1, 1]) == L.ERR_ARG and orders(n=2, comp=[2, 1]) == L.ERR_ARG
        assert orders(n=2, comp=[0, n]) == L.ERR_ARG and orders(n=1, comp=[-1]) == L.ERR_ARG
        assert orders(h=bare) == L.ERR_ARG                                                 # uv of a graph made without key points
        big = int(np.argmax(sizes))
        assert orders(n=1, comp=[big], attempt=int(sizes.max())) == L.ERR_ARG
        check_orders(g.orders([big], int(sizes.max()) - 1, uv=True), "thresholds", 3, int(sizes.max()) - 1, [big])
        check_orders(bare.orders(), "thresholds", 3, 0)
        with pytest.raises(ValueError, match="key points"):
            bare.orders(uv=True)
        off = np.full(n + 1, -7, np.int64)
        assert lib.lvba_trackgraph_components(g._h, None, None, None, None) == L.ERR_ARG
        assert lib.lvba_trackgraph_components(g._h, off.ctypes.data, None, None, None) == L.ERR_ARG and (off == -7).all()
        assert lib.lvba_trackgraph_components(None, off.ctypes.data, None, None, None) == L.ERR_ARG
    assert lib.lvba_trackgraph_destroy(None) == 0
    assert C.sizeof(L.TrackGraphInfo) == 64


@pytest.mark.parametrize("name", ("random", "thresholds", "four_views"))
def test_track_loop_with_stub_fusions(pkg, name):
    pl = tc.pipeline()
    c = tc.case(name)
    for kind in ("never", "second", "always"):
        stubs, seen = fuse_stubs()
        want = pl.build_tracks_and_fuse(c["keypoints"], c["pairs"], c["matches"], stubs[kind], 3)
        seen.clear()
        got = pl.build_tracks_and_fuse(c["keypoints"], c["pairs"], c["matches"], stubs[kind], 3, device_tracks=True)
        assert got.keys() == want.keys()
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name} {kind} {key}")


def test_track_loop_with_the_real_fusion(pkg):
    """the depth-guided matches of the facade's four views, fused by visual.fuse_tracks against its depth images.  The views stand
    0.5 - 1.05 m apart 8 m before the facade (3.6 - 7.5 degrees): at the reference's 8 degrees every component is dropped after all
    its attempts, at 3 degrees the points seen from views 0 - 2 are accepted; both loops are compared."""
    import match_depth_cases as mdc
    pl = tc.pipeline()
    V = importlib.import_module("global-lvba_amd.visual")
    f = mdc.facade()
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    descs, kps = f["descs"][:4], f["keypoints"][:4]
    with V.DepthImages.upload(f["depth"][:4]) as depth:
        matches = pl.match_image_pairs(descs, pairs, keypoints=kps, Rcw=f["Rcw"][:4], tcw=f["tcw"][:4], intr=f["intr"], depth=depth)

        def fuse_at(angle):
            return lambda o, i, u: V.fuse_tracks(o, i, u, f["Rcw"][:4], f["tcw"][:4], f["intr"], depth=depth, obser_thr=3,
                                                 min_view_angle_deg=angle, reproj_mean_thr_px=3.0)

        runs = [(pl.build_tracks_and_fuse(kps, pairs, matches, fuse_at(angle), 3),
                 pl.build_tracks_and_fuse(kps, pairs, matches, fuse_at(angle), 3, device_tracks=True)) for angle in (8.0, 3.0)]
    print([(len(w["X"]), len(w["component_status"]), int(w["attempts"].max(initial=0))) for w, _ in runs])
    assert len(runs[0][0]["X"]) == 0 and len(runs[0][0]["component_status"]) > 10 and len(runs[1][0]["X"]) > 10
    for want, got in runs:
        assert got.keys() == want.keys()
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_full_pipeline_with_device_tracks(pkg):
    """run_full_pipeline(match_fn=..., device_tracks=True) on the small sequence of the pipeline tests: the arrays of the visual
    stage are those of the default run"""
    import match_cases as mc
    import test_gpu_pipeline as tp
    pl = tc.pipeline()
    d = tp._dataset(n_frames=10, pts=20000, n_land=300, seed=64)
    rng = np.random.default_rng(64)
    tex = mc.sift_like(rng, len(d["X"]))
    descs = [mc.noisy(rng, tex[np.asarray(ids, np.int64)], 6) if len(ids) else np.zeros((0, 128), np.uint8) for ids in d["lm_of"]]

    def match_fn(cam_poses):
        Rcw, tcw = pl.camera_from_imu(cam_poses, tp.RCB, tp.TCI)
        return d["pairs"], pl.match_image_pairs(descs, d["pairs"], keypoints=d["kps"], Rcw=Rcw, tcw=tcw, intr=tp.INTR)

    def run(**kw):
        return pl.run_full_pipeline(d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"],
                                    [], [], match_fn=match_fn, window_size=5, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5),
                                    stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4), **kw)["visual"]

    want, got = run(), run(device_tracks=True)
    assert want["n_components"] > 0 and got.keys() == want.keys()
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            np.testing.assert_array_equal(got[key], w, err_msg=key)
    for key, w in want["tracks"].items():
        np.testing.assert_array_equal(got["tracks"][key], w, err_msg=f"tracks {key}")
