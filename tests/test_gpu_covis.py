"""GPU tests of the co-visibility pair selection (lvba_covis_samples / _counts / _pairs; covis.py, pipeline.select_image_pairs,
run_full_pipeline(match_select=...)) against the numpy restatement (tests/covis_oracle.py) on the room fixture
(tests/covis_cases.py).  Every comparison is exact: the samples are multiplications, additions and correctly
rounded divisions of correctly rounded operands, and the fixture keeps every decision at least 1e-9 away from its bound
(test_covis_host.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import covis_cases as cc
import match_cases as mc

pytestmark = pytest.mark.gpu

SHAPES = [(size, grid) for size in range(len(cc.SIZES)) for grid in range(len(cc.GRIDS))]
SHAPE_IDS = [f"{cc.SIZES[s][0]}x{cc.SIZES[s][1]}-grid{cc.GRIDS[g][0]}x{cc.GRIDS[g][1]}" for s, g in SHAPES]


@pytest.fixture(scope="module")
def CV(pkg):
    return importlib.import_module("global-lvba_amd.covis")


@pytest.fixture(scope="module")
def depths(pkg):
    """(size, M) -> (the first M depth images on the device, Rcw, tcw, intr)"""
    V = importlib.import_module("global-lvba_amd.visual")
    held = {}
    for size in range(len(cc.SIZES)):
        r = cc.room(size)
        for M in cc.M_VALUES:
            held[(size, M)] = (V.DepthImages.upload(r["depth"][:M]), r["Rcw"][:M], r["tcw"][:M], r["intr"])
    yield held
    for d in held.values():
        d[0].close()


@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_samples_equal_the_oracle(CV, depths, size):
    for grid in range(len(cc.GRIDS)):
        for M in cc.M_VALUES:
            got = CV.samples(*depths[(size, M)], **cc.grid_opts(grid))
            want, _ = cc.lifted(size, grid, M)
            assert got.shape == want.shape
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            np.testing.assert_array_equal(got, want)
    assert 0 < np.isnan(cc.lifted(size, 0)[0][:, :, 0]).sum() < cc.N_IMAGES * 192


@pytest.mark.parametrize("size, grid", SHAPES, ids=SHAPE_IDS)
def test_counts_equal_the_oracle(CV, depths, size, grid):
    for occlusion in (0, 1):
        for M in cc.M_VALUES:
            n, c = CV.counts(*depths[(size, M)], occlusion=occlusion, **cc.grid_opts(grid))
            _, _, wn, wc = cc.judged(size, grid, occlusion, M)
            np.testing.assert_array_equal(n, wn, err_msg=f"occlusion {occlusion}, M {M}")
            np.testing.assert_array_equal(c, wc, err_msg=f"occlusion {occlusion}, M {M}")
            assert n.dtype == c.dtype == np.int32 and c.shape == (M, M) and not np.diag(c).any()


@pytest.mark.parametrize("kw", cc.OPTION_SETS, ids=[str(i) for i in range(len(cc.OPTION_SETS))])
def test_pairs_equal_the_oracle(CV, depths, kw):
    for size, grid in SHAPES:
        for M in cc.M_VALUES:
            got = CV.select_pairs(*depths[(size, M)], **cc.grid_opts(grid), **kw)
            want = cc.selected(size, grid, M, **kw)
            for g, w, name in zip(got, want, ("pairs", "score", "shared")):
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(g, w, err_msg=f"{name}: {cc.SIZES[size]}, grid {cc.GRIDS[grid]}, M {M}")
            if M == 1:
                assert len(got[0]) == 0
    again = CV.select_pairs(*depths[(0, cc.N_IMAGES)], **cc.grid_opts(0), **kw)           # the same bytes on a second call
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, CV.select_pairs(*depths[(0, cc.N_IMAGES)], **cc.grid_opts(0), **kw)))
    assert len(again[0]) > 0


def raw_pairs(CV, held, capacity, pairs, score, shared, **kw):
    d, R, t, intr = held
    o = CV.covis_opts(**kw)
    count = C.c_int64(-7)
    rc = d.lib.lvba_covis_pairs(d._h, np.ascontiguousarray(R).ctypes.data, np.ascontiguousarray(t).ctypes.data, intr.ctypes.data, C.byref(o),
                                capacity, None if pairs is None else pairs.ctypes.data, None if score is None else score.ctypes.data,
                                None if shared is None else shared.ctypes.data, C.byref(count))
    return rc, count.value


def test_capacity_below_count_writes_the_prefix(pkg, CV, depths):
    L = pkg._lib
    held = depths[(0, cc.N_IMAGES)]
    wp, ws, wsh = cc.selected(0, 0)
    assert len(wp) > 12
    for cap in (1, 7, len(wp) - 1, len(wp), len(wp) + 5):
        pairs, score, shared = np.full((len(wp) + 8, 2), -7, np.int32), np.full(len(wp) + 8, -7.0), np.full((len(wp) + 8, 2), -7, np.int32)
        rc, count = raw_pairs(CV, held, cap, pairs, score, shared)
        assert rc == L.OK and count == len(wp)
        k = min(cap, len(wp))
        np.testing.assert_array_equal(pairs[:k], wp[:k]); np.testing.assert_array_equal(score[:k], ws[:k])
        np.testing.assert_array_equal(shared[:k], wsh[:k])
        assert (pairs[k:] == -7).all() and (score[k:] == -7.0).all() and (shared[k:] == -7).all()    # the rest is untouched
    # capacity = 0 with null outputs: the count alone; score and shared are optional at any capacity
    assert raw_pairs(CV, held, 0, None, None, None) == (L.OK, len(wp))
    pairs = np.full((len(wp), 2), -7, np.int32)
    assert raw_pairs(CV, held, len(wp), pairs, None, None) == (L.OK, len(wp))
    np.testing.assert_array_equal(pairs, wp)
    # the Python wrapper asks again when its guess was too small
    got = CV.select_pairs(*held, capacity=3)
    np.testing.assert_array_equal(got[0], wp); np.testing.assert_array_equal(got[1], ws); np.testing.assert_array_equal(got[2], wsh)
    assert raw_pairs(CV, depths[(0, 1)], 4, np.full((4, 2), -7, np.int32), None, None) == (L.OK, 0)       # M = 1


def test_refused_calls_write_nothing(pkg, CV, depths):
    L = pkg._lib
    V = importlib.import_module("global-lvba_amd.visual")
    d, R, t, intr = depths[(1, cc.N_IMAGES)]                                             # 37 x 29
    M, lib = cc.N_IMAGES, d.lib
    R, t = np.ascontiguousarray(R), np.ascontiguousarray(t)

    def all_three(want, handle=d._h, R=R, t=t, intr=intr, opts=None, M=M, G=192, calls="scp", null=(), capacity=8):
        """the calls named in `calls` (samples, counts, pairs) with these arguments; every output starts at -7 and must still hold it"""
        o = C.byref(opts) if opts is not None else None
        a = [handle] + [None if x is None else x.ctypes.data for x in (R, t, intr)] + [o]
        world, n, c = np.full((M, G, 3), -7.0), np.full(M, -7, np.int32), np.full((min(M, 64), min(M, 64)), -7, np.int32)
        pairs, score, shared, count = np.full((8, 2), -7, np.int32), np.full(8, -7.0), np.full((8, 2), -7, np.int32), C.c_int64(-7)
        p = lambda x, name: None if name in null else x.ctypes.data
        if "s" in calls:
            assert lib.lvba_covis_samples(*a, p(world, "world")) == want
        if "c" in calls:
            assert lib.lvba_covis_counts(*a, p(n, "n_points"), p(c, "counts")) == want
        if "p" in calls:
            assert lib.lvba_covis_pairs(*a, capacity, p(pairs, "pairs"), score.ctypes.data, shared.ctypes.data,
                                        None if "count" in null else C.byref(count)) == want
        assert (world == -7.0).all() and (n == -7).all() and (c == -7).all() and (pairs == -7).all() and (score == -7.0).all()
        assert (shared == -7).all() and count.value == -7

    # a null required pointer
    all_three(L.ERR_ARG, handle=None)
    all_three(L.ERR_ARG, R=None)
    all_three(L.ERR_ARG, t=None)
    all_three(L.ERR_ARG, intr=None)
    all_three(L.ERR_ARG, calls="s", null=("world",))
    all_three(L.ERR_ARG, calls="c", null=("n_points",))
    all_three(L.ERR_ARG, calls="c", null=("counts",))
    all_three(L.ERR_ARG, calls="p", null=("count",))
    all_three(L.ERR_ARG, calls="p", null=("pairs",))                                     # capacity > 0 with pairs null
    all_three(L.ERR_ARG, calls="p", capacity=-1)
    # a non-finite pose or intrinsic
    for k, v in ((0, np.nan), (9 * M - 1, np.inf)):
        bad = R.copy(); bad.reshape(-1)[k] = v
        all_three(L.ERR_ARG, R=bad)
    bad = t.copy(); bad[M // 2, 1] = -np.inf
    all_three(L.ERR_ARG, t=bad)
    for k in (0, 7):
        bad = intr.copy(); bad[k] = np.nan
        all_three(L.ERR_ARG, intr=bad)
    # an option outside its range, and a grid finer than the image
    for kw in (dict(grid_x=0), dict(grid_x=65), dict(grid_y=0), dict(grid_y=65), dict(search_radius=-1), dict(search_radius=17),
               dict(occlusion=2), dict(occlusion=-1), dict(both_ways=2), dict(max_per_image=-1), dict(max_per_image=1025), dict(min_shared=-1),
               dict(min_overlap=np.nan), dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(occlusion_rel=-1e-3), dict(occlusion_rel=np.inf),
               dict(occlusion_abs=np.nan), dict(occlusion_abs=-1.0), dict(grid_x=37), dict(grid_y=29), dict(grid_x=64, grid_y=64)):
        all_three(L.ERR_ARG, opts=CV.covis_opts(**kw))
    assert b"grid" in lib.lvba_last_error()
    # the largest grid the image admits is served
    assert CV.samples(d, R, t, intr, grid_x=36, grid_y=28).shape == (M, 36 * 28, 3)
    # more images than the count matrix is allowed to hold
    many = 8193
    with V.DepthImages.upload(np.ones((many, 2, 2), np.float32)) as big:
        Rb, tb = np.ascontiguousarray(np.broadcast_to(np.eye(3), (many, 3, 3))), np.zeros((many, 3))
        all_three(L.ERR_UNSUPPORTED, handle=big._h, R=Rb, t=tb, opts=CV.covis_opts(grid_x=1, grid_y=1), M=many, G=1)
    o = CV.covis_opts()
    assert C.sizeof(L.CovisOpts) == 56 and (o.grid_x, o.grid_y, o.search_radius, o.occlusion, o.both_ways, o.max_per_image, o.min_shared) == \
        (16, 12, 4, 1, 0, 0, 8) and (o.min_overlap, o.occlusion_rel, o.occlusion_abs) == (0.1, 0.05, 0.1)
    with pytest.raises(TypeError):
        CV.covis_opts(grid=3)


def test_select_image_pairs_adds_the_sequential_pairs(pkg, depths):
    pl = importlib.import_module("global-lvba_amd.pipeline")
    M = cc.N_IMAGES
    wp = [tuple(p) for p in cc.selected(0, 0)[0].tolist()]
    pairs, report = pl.select_image_pairs(*depths[(0, M)])
    assert pairs == wp and report == dict(n_images=M, all_pairs=M * (M - 1) // 2, selected=len(wp), covisible=len(wp), empty_images=[cc.EMPTY])
    pairs, report = pl.select_image_pairs(*depths[(0, M)], sequential=1)
    chain = {(i, i + 1) for i in range(M - 1)}
    assert pairs == sorted(set(wp) | chain) and not chain <= set(wp)
    assert (cc.EMPTY - 1, cc.EMPTY) in pairs and report["selected"] == len(pairs) > report["covisible"] == len(wp)
    pairs, report = pl.select_image_pairs(*depths[(0, M)], sequential=2, max_per_image=1, **cc.grid_opts(2))
    want = {tuple(p) for p in cc.selected(0, 2, max_per_image=1)[0].tolist()} | {(i, j) for i in range(M) for j in range(i + 1, min(M, i + 3))}
    assert pairs == sorted(want)
    assert pl.select_image_pairs(*depths[(0, 1)], sequential=3) == ([], dict(n_images=1, all_pairs=0, selected=0, covisible=0, empty_images=[]))


def test_full_pipeline_with_match_select(pkg, monkeypatch):
    """run_full_pipeline(match_fn=..., match_select=True) on the small sequence of the pipeline tests: the matcher is handed the
    selected pairs, the depth images are rendered once and shared with the visual stage, and the visual stage runs."""
    import test_gpu_pipeline as tp
    pl = importlib.import_module("global-lvba_amd.pipeline")
    vis = importlib.import_module("global-lvba_amd.visual")
    d = tp._dataset(n_frames=10, pts=20000, n_land=300, seed=64)
    rng = np.random.default_rng(64)
    tex = mc.sift_like(rng, len(d["X"]))
    descs = [mc.noisy(rng, tex[np.asarray(ids, np.int64)], 6) if len(ids) else np.zeros((0, 128), np.uint8) for ids in d["lm_of"]]
    handed, chosen, renders = [], [], []
    render, select = vis.DepthImages.render, pl.select_image_pairs

    def match_fn(cam_poses, pairs=None, depth=None):
        handed.append((pairs, depth))
        Rcw, tcw = pl.camera_from_imu(cam_poses, tp.RCB, tp.TCI)
        return pairs, pl.match_image_pairs(descs, pairs, keypoints=d["kps"], Rcw=Rcw, tcw=tcw, intr=tp.INTR, depth=depth)

    def recording_select(*a, **k):
        chosen.append(select(*a, **k))
        return chosen[-1]

    def counting_render(*a, **k):
        renders.append(1)
        return render(*a, **k)

    monkeypatch.setattr(vis.DepthImages, "render", counting_render)
    monkeypatch.setattr(pl, "select_image_pairs", recording_select)
    M = len(d["img_t"])
    for extra in (dict(match_select=True), dict(match_select=dict(sequential=1, min_overlap=0.2), match_depth=True)):
        del handed[:], chosen[:], renders[:]
        out = pl.run_full_pipeline(d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"],
                                   [], [], match_fn=match_fn, window_size=5, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5),
                                   stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4), **extra)
        assert len(handed) == len(chosen) == len(renders) == 1                 # rendered once, shared with the visual stage
        pairs, report = chosen[0]
        assert handed[0][0] is pairs and (handed[0][1] is not None) == ("match_depth" in extra)
        assert out["pair_selection"] == report and out["pairs"] is pairs and len(out["matches"]) == len(pairs)
        assert report["n_images"] == M and report["all_pairs"] == M * (M - 1) // 2 and 0 < report["selected"] == len(pairs) <= report["all_pairs"]
        assert all(0 <= i < j < M for i, j in pairs) and pairs == sorted(pairs)
        if "match_depth" in extra:
            assert {(i, i + 1) for i in range(M - 1)} <= set(pairs)
        assert sum(len(m) for m in out["matches"]) > 0
        v = out["visual"]
        assert v["n_components"] > 0 and "termination" in v
