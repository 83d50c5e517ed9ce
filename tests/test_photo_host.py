"""CPU tests of the multi-view colour fusion (include/lvba_hip.h "multi-view colour fusion and photometric consistency", DESIGN.md
§10p): the numpy oracle against the rule as plain loops, the fixture's margin condition, the device header compiled for the host
against the oracle bit for bit, the overflow bounds hit exactly, the claim -- the spread separates planted cameras from turned
ones and an occlusion test from none --, a closed form that needs no oracle, and the wiring of the pipeline."""
import ctypes
import importlib
import json
import math
import sqlite3
import sys

import numpy as np
import pytest

import covis_cases as cc
import match_cases as mc
import photo_cases as pc
import photo_oracle as po
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/photo_device.h compiled for the host, without contraction (tests/photo_check.cpp)"""
    lib = ctypes.CDLL(build_check("photo_check", tmp_path_factory.mktemp("emul_photo")))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.emul_sums.argtypes = [ctypes.c_int64, P, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.emul_repeat.argtypes = [P, I, P, P, P]
    lib.emul_finish.argtypes = [ctypes.c_int64, P, P, P, I, P, P]
    lib.emul_sums.restype = lib.emul_repeat.restype = lib.emul_finish.restype = None
    return lib


def ptr(x):
    return x.ctypes.data


def host_sums(emul, points, images, depth, intr, Rcw, tcw, **kw):
    o = dict(po.DEFAULTS, **kw)
    M, H, W = images.shape[:3]
    n = len(points)
    seen, c16 = np.zeros((M, n), np.uint8), np.zeros((M, n, 3), np.int32)
    nv, s1, s2 = np.zeros(n, np.int32), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.int64)
    bounds = np.array([o["occlusion_rel"], o["occlusion_abs"], o["max_depth"]], np.float64)
    flags = np.array([o["holes"], o["min_views"]], np.int32)
    emul.emul_sums(n, ptr(points), M, W, H, None if depth is None else ptr(depth), ptr(np.ascontiguousarray(Rcw)),
                   ptr(np.ascontiguousarray(tcw)), ptr(images), ptr(np.ascontiguousarray(intr, np.float64)), ptr(bounds), ptr(flags),
                   ptr(seen), ptr(c16), ptr(nv), ptr(s1), ptr(s2))
    return seen.astype(bool), c16, nv, s1, s2


def host_finish(emul, nv, s1, s2, min_views=2):
    n = len(nv)
    rgb, sigma = np.zeros((n, 3), np.uint8), np.zeros(n)
    emul.emul_finish(n, ptr(np.ascontiguousarray(nv, np.int32)), ptr(np.ascontiguousarray(s1, np.uint32)),
                     ptr(np.ascontiguousarray(s2, np.int64)), min_views, ptr(rgb), ptr(sigma))
    return rgb, sigma


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_oracle_equals_the_rule_as_loops():
    """the 37 x 29 images, every 7th point, all 21 images, every option set: sums and finish"""
    s = pc.scene(1)
    take = np.arange(0, cc.N_PLANTED, 7)
    for kw in pc.OPTION_SETS:
        with_depth, opts = pc.split(kw)
        e = pc.expected(1, **kw)
        want = po.loops_sums(s["points"][take], s["images"], s["depth"] if with_depth else None, s["intr"], s["Rcw"], s["tcw"], **opts)
        assert [w[0] for w in want] == e["n_views"][take].tolist(), kw
        assert [w[1] for w in want] == e["s1"][take].tolist() and [w[2] for w in want] == e["s2"][take].tolist(), kw
        for k, (n, s1, s2) in zip(take, want):
            rgb, sigma = po.loops_finish(n, s1, s2, **opts)
            assert rgb == e["rgb"][k].tolist(), (kw, k)
            assert np.float64(sigma).tobytes() == e["sigma"][k].tobytes(), (kw, k)


def test_fixture_conditions():
    worst = pc.check_margins()
    assert worst["compare"] >= mc.MIN_MARGIN and worst["texel"] >= pc.TEXEL_MARGIN
    for size in range(len(cc.SIZES)):
        e = pc.expected(size)
        nv = e["n_views"]
        assert (nv == 0).any() and (nv == 1).any() and (nv >= 3).any()          # every branch of the finish
        assert np.isnan(e["sigma"][nv < 2]).all() and np.isfinite(e["sigma"][nv >= 2]).all()
        assert not e["seen"][cc.EMPTY].any() and e["seen"][cc.TWIN].tobytes() == e["seen"][0].tobytes()
        summaries = [json.dumps(pc.expected(size, **kw)["summary"], sort_keys=True) for kw in pc.OPTION_SETS]
        assert len(set(summaries)) == len(summaries)                             # the option sets do sample different things
        assert pc.expected(size, holes=1)["seen"][cc.EMPTY].any()                # a hole counts once it is allowed to


def test_device_header_on_the_host_equals_the_oracle(emul):
    """every sample and every finish, bit for bit, on both sizes and every option set the GPU tests use"""
    for size in range(len(cc.SIZES)):
        s = pc.scene(size)
        X = s["points"].astype(np.float64)
        for kw in pc.OPTION_SETS:
            with_depth, opts = pc.split(kw)
            e = pc.expected(size, **kw)
            depth = s["depth"] if with_depth else None
            seen, c16, nv, s1, s2 = host_sums(emul, s["points"], s["images"], depth, s["intr"], s["Rcw"], s["tcw"], **opts)
            assert same_bytes(seen, e["seen"]), (size, kw)
            for j in range(cc.N_IMAGES):
                _, want, _ = po.sample_image(X, s["images"][j], None if depth is None else depth[j], s["intr"], s["Rcw"][j], s["tcw"][j], **opts)
                np.testing.assert_array_equal(c16[j], want, err_msg=f"{size} {kw} image {j}")
            assert same_bytes(nv, e["n_views"]) and same_bytes(s1, e["s1"]) and same_bytes(s2, e["s2"]), (size, kw)
            rgb, sigma = host_finish(emul, nv, s1, s2, dict(po.DEFAULTS, **opts)["min_views"])
            assert same_bytes(rgb, e["rgb"]) and same_bytes(sigma, e["sigma"]), (size, kw)


def test_pixel_edges_on_the_host(emul):
    """the exact-arithmetic case of the GPU test, header against oracle, and the edges themselves"""
    c = pc.pixel_edge_case()
    R, t = np.eye(3)[None], np.zeros((1, 3))
    e = po.evaluate(c["points"], c["image"], None, c["intr"], R, t)
    seen, c16, nv, s1, s2 = host_sums(emul, c["points"], c["image"], None, c["intr"], R, t)
    assert same_bytes(seen, e["seen"]) and same_bytes(s1, e["s1"]) and same_bytes(s2, e["s2"])
    u, v = c["u"], c["v"]
    inside = (u >= 0) & (u < c["W"] - 1) & (v >= 0) & (v < c["H"] - 1)
    np.testing.assert_array_equal(seen[0], inside)
    assert seen[0][(u == 0) & (v == 0)].all() and not seen[0][u == c["W"] - 1].any() and not seen[0][v == c["H"] - 1].any()
    assert not seen[0][-2:].any()                                               # Z = 0 and behind the camera


def test_overflow_bounds_are_hit_exactly(emul):
    """32 768 views of an all-255 image on one point: S1 = 32 768 * 65 280, N_c = 0, sigma = 0"""
    img = np.full((1, 4, 4, 3), 255, np.uint8)
    pts = np.array([[0.0, 0.0, 1.0]], np.float32)
    intr = np.array([2.0, 2.0, 1.3, 1.3, 0, 0, 0, 0])
    _, c16, _, _, _ = host_sums(emul, pts, img, None, intr, np.eye(3)[None], np.zeros((1, 3)))
    assert c16[0, 0].tolist() == [65280] * 3
    nv, s1, s2 = np.zeros(1, np.int32), np.zeros((1, 3), np.uint32), np.zeros((1, 3), np.int64)
    emul.emul_repeat(ptr(np.ascontiguousarray(c16[0, 0])), 32768, ptr(nv), ptr(s1), ptr(s2))
    assert nv[0] == 32768 and s1[0].tolist() == [32768 * 65280] * 3 and s2[0].tolist() == [32768 * 65280 ** 2] * 3
    assert 32768 * int(s2[0, 0]) < 2 ** 63 and int(s1[0, 0]) < 2 ** 31
    rgb, sigma = host_finish(emul, nv, s1, s2)
    assert rgb[0].tolist() == [255] * 3 and sigma[0] == 0.0
    rgb, sigma = po.finish(nv, s1, s2)
    assert rgb[0].tolist() == [255] * 3 and sigma[0] == 0.0
    # the largest variance the sums can hold: half the views at 0, half at 65 280
    half = np.array([[16384 * 65280] * 3], np.uint32)
    s2h = np.array([[16384 * 65280 ** 2] * 3], np.int64)
    rgb, sigma = host_finish(emul, nv, half, s2h)
    assert sigma[0] == 127.5 and rgb[0].tolist() == [128] * 3                  # (2 * 32640 + 256) // 512 = 128: round half up
    assert same_bytes(po.finish(nv, half, s2h)[1], sigma)


def mean_sigma(s, R, t, depth):
    N = cc.N_CAMERAS
    return po.evaluate(s["points"], s["images"][:N], depth, s["intr"], R, t)["summary"]["mean_sigma"]


def test_the_measure_means_something():
    """orderings on the oracle over the 18 cameras (the values are in DESIGN.md §10p): planted < each turned by 0.5 degrees < by
    2 degrees, depth images re-rendered at the turned cameras; occlusion test on < off; and the fused colour is the planted one"""
    N = cc.N_CAMERAS
    for size in range(len(cc.SIZES)):
        s = pc.scene(size)
        planted = mean_sigma(s, s["Rcw"][:N], s["tcw"][:N], s["depth"][:N])
        half = mean_sigma(s, *pc.turned(size, 0.5, 11))
        two = mean_sigma(s, *pc.turned(size, 2.0, 11))
        blind = mean_sigma(s, s["Rcw"][:N], s["tcw"][:N], None)
        e = pc.expected(size)
        v = e["n_views"] > 0
        err = np.median(np.abs(e["rgb"][v].astype(np.float64) - s["colour"][v][:, ::-1]))
        print(f"size {cc.SIZES[size]}: mean spread planted {planted:.3f}, turned 0.5 deg {half:.3f}, 2 deg {two:.3f}, no occlusion test "
              f"{blind:.3f} grey levels; median channel error of the fused colour {err:.3f}")
        assert planted < half < two and planted < blind
        assert err < 2.0          # byte rounding of the image, the 1/256 quantisation, interpolation of a smooth texture over a pixel


def test_constant_colour_closed_form(emul):
    """image k one colour: every sample is exactly 256 colour, so sums, rgb and sigma of a point follow from which images see it"""
    for size in range(len(cc.SIZES)):
        s = pc.scene(size)
        img, colours = pc.constant_images(size)
        seen, c16, nv, s1, s2 = host_sums(emul, s["points"], img, s["depth"], s["intr"], s["Rcw"], s["tcw"])
        assert same_bytes(seen, pc.expected(size)["seen"])                      # which images see a point does not depend on the colours
        for j in range(cc.N_IMAGES):
            assert (c16[j][seen[j]] == 256 * colours[j]).all()
        n, S1, S2, rgb, N = pc.closed_form(seen, colours)
        assert same_bytes(nv, n) and same_bytes(s1, S1) and same_bytes(s2, S2)
        got_rgb, got_sigma = host_finish(emul, nv, s1, s2)
        assert same_bytes(got_rgb, rgb)
        for k in np.flatnonzero(n >= 2)[::5]:
            want = math.sqrt(((float(N[k, 0]) + float(N[k, 1])) + float(N[k, 2])) / (3.0 * 65536.0 * float(int(n[k]) ** 2)))
            assert got_sigma[k] == want
        assert np.isnan(got_sigma[n < 2]).all()


def test_struct_sizes_and_defaults(pkg):
    L = pkg._lib
    assert ctypes.sizeof(L.PhotoOpts) == 40 and ctypes.sizeof(L.PhotoSummary) == 80
    PH = importlib.import_module("global-lvba_amd.photo")
    import __graft_entry__ as ge
    ge.build()
    o = PH.photo_opts()
    assert {k: getattr(o, k) for k in PH.OPTION_NAMES} == po.DEFAULTS
    with pytest.raises(TypeError, match="photometric consistency"):
        PH.photo_opts(no_such=1)


class _FakeScans:
    device = 0

    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


ARGS = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
        np.ones(8), 640, 512, [np.zeros((5, 2), np.float32)] * 2, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])


def test_the_default_path_calls_no_photo_entry_point(monkeypatch):
    """photo_consistency=None (the default) neither imports the photo module nor looks an lvba_photo_* symbol up, with and without
    images; and the keyword without images is refused"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")

    class NoPhotoLib:
        def __getattr__(self, name):
            if name.startswith("lvba_photo"):
                pytest.fail(f"{name} looked up on the default path")
            raise AttributeError(name)

    visual = dict(Rcw=np.zeros((2, 3, 3)), tcw=np.zeros((2, 3)), Rcw_before=np.zeros((2, 3, 3)), tcw_before=np.zeros((2, 3)))
    cloud = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: dict(visual))
    monkeypatch.setattr(pl, "colorize_maps", lambda *a, **k: dict(after=cloud, before=cloud))
    monkeypatch.setattr(pl, "_photo_consistency", lambda *a, **k: pytest.fail("the stage ran on the default path"))
    monkeypatch.setattr(L, "load", lambda: NoPhotoLib())
    sys.modules.pop("global-lvba_amd.photo", None)
    for kw in (dict(), dict(images=np.zeros((2, 512, 640, 3), np.uint8)), dict(photo_consistency=None), dict(photo_consistency=False)):
        out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, **kw)
        assert not [k for k in out if k.startswith(("photo", "fused"))]
    assert "global-lvba_amd.photo" not in sys.modules
    with pytest.raises(ValueError, match="images"):
        pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, photo_consistency=True)


def test_run_full_pipeline_hands_the_coloured_points_on(monkeypatch):
    """the after set goes with the refined poses and cameras and colored_after's points, the before set with the original ones;
    the output holds the summaries and the fused maps on the coloured maps' points"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    visual = dict(Rcw=np.ones((2, 3, 3)), tcw=np.ones((2, 3)), Rcw_before=np.zeros((2, 3, 3)), tcw_before=np.zeros((2, 3)))
    after, before = (np.ones((4, 3), np.float32), np.zeros((4, 3), np.uint8)), (np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    calls = []

    def fake(scans, scan_times, image_times, images, intr, width, height, after, before, points_after, points_before, **kw):
        calls.append((after, before, points_after, points_before, kw))
        one = lambda p, tag: dict(summary=dict(n_points=len(p), mean_sigma=tag), n_views=np.zeros(len(p), np.int32),
                                  rgb=np.zeros((len(p), 3), np.uint8), sigma=np.zeros(len(p)), options=dict(min_views=3))
        return dict(after=one(points_after, 1.0), before=one(points_before, 2.0))

    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: dict(visual))
    monkeypatch.setattr(pl, "colorize_maps", lambda *a, **k: dict(after=after, before=before))
    monkeypatch.setattr(pl, "_photo_consistency", fake)
    out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=np.zeros((2, 512, 640, 3), np.uint8), photo_consistency=dict(min_views=3))
    (a, b, pa, pb, kw), = calls
    assert a[1] is visual["Rcw"] and b[1] is visual["Rcw_before"] and pa is after[0] and pb is before[0]
    assert kw == dict(min_views=3, depth_half_window_s=pl.DEFAULTS["depth_half_window_s"], depth_voxel=pl.DEFAULTS["depth_voxel"])
    assert out["photo_consistency"] == dict(after=dict(n_points=4, mean_sigma=1.0), before=dict(n_points=5, mean_sigma=2.0))
    assert out["fused_after"][0] is after[0] and len(out["fused_after"]) == 4 and out["fused_before"][0] is before[0]
    assert out["fused_after"][1].shape == (4, 3) and out["fused_before"][3].shape == (5,)


def test_run_dataset_hands_the_keyword_on_and_writes_the_report(tmp_path, monkeypatch):
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    for t in (0.5, 1.5):
        ds.save_pcd(str(tmp_path / "all_pcd_body" / f"{t}.pcd"), rng.normal(size=(10, 4)).astype(np.float32))
        (tmp_path / "all_image" / f"{t}.png").write_bytes(b"")
    (tmp_path / "all_pcd_body" / "lidar_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    (tmp_path / "all_image" / "image_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    con = sqlite3.connect(str(tmp_path / "db.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    kp = rng.uniform(0, 500, (6, 4)).astype(np.float32)
    for iid, name in ((1, "0.500000.png"), (2, "1.500000.png")):
        con.execute("INSERT INTO images VALUES (?, ?)", (iid, name))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (iid, 6, 4, kp.tobytes()))
    con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                (ds.image_ids_to_pair_id(1, 2), 2, 2, np.array([[0, 1], [2, 3]], np.uint32).tobytes()))
    con.commit(); con.close()
    summary = dict(n_points=4, n_seen=3, n_valid=2, n_samples=7, mean_sigma=0.5, mean_views=7 / 3, ms=[0.1, 0.2, 0.3, 0.4])
    options = dict(po.DEFAULTS, min_views=3)
    calls = []

    def full_pipeline(*a, **k):
        calls.append(k)
        extra = dict(photo_consistency=dict(after=summary, before=dict(summary, mean_sigma=0.75)), photo_options=options) \
            if k.get("photo_consistency") else {}
        return dict(extra, poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1)))

    monkeypatch.setattr(pl, "run_full_pipeline", full_pipeline)
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir))
    assert "photo_consistency" not in calls[0] and calls[0]["images"] is None and not (out_dir / "photo_consistency.json").exists()
    pl.run_dataset(*args, out_dir=str(out_dir), photo_consistency=dict(min_views=3))
    assert calls[1]["photo_consistency"] == dict(min_views=3) and callable(calls[1]["images"])      # the images are read without colorize=True
    rep = json.load(open(out_dir / "photo_consistency.json"))
    assert sorted(rep) == ["after", "before", "options"]
    assert rep["after"] == summary and rep["before"]["mean_sigma"] == 0.75 and rep["options"] == options
    assert sorted(rep["after"]) == sorted(["n_points", "n_seen", "n_valid", "n_samples", "mean_sigma", "mean_views", "ms"])
