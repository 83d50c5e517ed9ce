"""CPU tests (no GPU) of tests/fusion_cases.py: every depth case's oracle image against the pixel lists derived by hand, every
track case through the host build of the device header (tests/host_emul_tracks.cpp: the very fuse_track the kernel runs)
against the oracle at the bars of tests/test_gpu_fusion.py, and the conditions the cases are built to meet, read from the
oracle's trace: no decision of any track is within rounding of going the other way, and every outcome a case names occurs.
The two refusals of the entry points (a bad obs_off, a bad option) come before any device work and are asserted here too."""
import numpy as np
import pytest

from oracle import fusion_oracle as fo

import fusion_cases as fc
import test_tracks_host as TH

DEPTH = {c["name"]: c for c in fc.depth_cases()}
TRACKS = ("block_edges", "short_and_empty", "image_counts", "bucket_collisions", "long_track", "pixel_edges", "anchor", "selection")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return TH.build_emul(tmp_path_factory.mktemp("emul_fusion_cases"))


@pytest.mark.parametrize("name", sorted(DEPTH))
def test_depth_case_lists_hold_for_the_oracle(name):
    c = DEPTH[name]
    img = fc.oracle_depth(c)
    fc.check_depth_lists(c, img)
    if name.startswith("sizes_"):                                            # every point is in the frame: none is lost to it
        assert all((i > 0).any() for i in img)
    if name == "distorted_off_axis":
        assert (img[0] > 0).sum() > 50 and 0 < (img[1] > 0).sum() < (img[0] > 0).sum()


@pytest.mark.parametrize("axis", range(3))
def test_voxel_key_case_sits_on_the_rule(axis):
    c = DEPTH["voxel_key_axis%d" % axis]
    p = c["key_points"]
    assert fo.voxel_keys(p, 0.5)[:, axis].tolist() == [-2, -2, -1]
    assert np.floor(p[:, axis] / 0.5).tolist() == [-1, -2, -1]              # the rule it is not


def test_contention_case_is_what_it_says():
    c = DEPTH["one_pixel_contention"]
    world = np.concatenate([cl.astype(np.float64) + T[9:] for cl, T in zip(c["clouds"], c["scan_poses"])])
    u, v = 64.0 * world[:, 0] / world[:, 2] + 32.0, 64.0 * world[:, 1] / world[:, 2] + 24.0
    on = (u.astype(int) == 32) & (v.astype(int) == 24)
    z = world[on, 2].astype(np.float32)
    assert on.sum() == 4096 and (z == z.min()).sum() == 16 and len(np.unique(z)) == 4081
    assert len({tuple(k) for k in fo.voxel_keys(world[on], 0.5)}) >= 8 and ((u.astype(int) == 10) & (v.astype(int) == 10)).sum() == 2


def _runs(c):
    """(with_depth, options) of every run the tests make of a case."""
    sets = c.get("option_sets", ({},))
    return [(d, o) for o in sets for d in (True, False)]


@pytest.mark.parametrize("name", TRACKS + ("options",))
def test_device_header_matches_oracle(emul, name):
    c = fc.case_by_name(name)
    for with_depth, o in _runs(c):
        want = fc.oracle_tracks(c, with_depth, **o)
        got = TH._fuse(emul, c["off"], c["img"], c["uv"], c["depth"] if with_depth else None, c["Rcw"], c["tcw"], c["intr"],
                       obser_thr=o.get("obser_thr", 3), angle=o.get("min_view_angle_deg", 8.0), thr=o.get("reproj_mean_thr_px", 3.0))
        fc.assert_tracks_match(got, want, (name, with_depth, o))
        fc.check_track_lists(c, got, with_depth)


@pytest.mark.parametrize("name", TRACKS + ("options",))
def test_no_decision_is_within_rounding(name):
    """fp64 rounding of sums of <= 1e3 terms of magnitude <= 1e3 is ~1e-10 at worst: a mean 1e-6 px from the threshold and from
    the other candidate's, a dot product or a distance 1e-9 from its bound cannot fall the other way in a correct
    implementation.  Every track of every case, none left out."""
    c = fc.case_by_name(name)
    for with_depth, o in _runs(c):
        thr = o.get("reproj_mean_thr_px", 3.0)
        for t, tr in enumerate(fc.oracle_tracks(c, with_depth, **o)[4]):
            if not tr:
                continue
            means = [m for m in (tr["m_depth"], tr["m_tri"]) if m is not None]
            assert all(abs(m - thr) >= 1e-6 for m in means), (name, t, means)
            assert len(means) < 2 or abs(means[0] - means[1]) >= 1e-6, (name, t, means)
            assert all(abs(v) >= 1e-9 for v in tr["dot_margins"] + tr["dist_margins"]), (name, t)


def test_named_outcomes_occur():
    for name in TRACKS:
        c = fc.case_by_name(name)
        for d in (True, False):
            fc.check_track_lists(c, fc.oracle_tracks(c, d), d)
    c = fc.case_by_name("image_counts")
    tr = fc.oracle_tracks(c, True)[4][c["keeps_three"]]
    assert tr["n_kept_depth"] == 3 and tr["n_kept_tri"] == 3
    c = fc.case_by_name("anchor")
    st, _, _, _, traces = fc.oracle_tracks(c, True)
    for t in c["wrong_anchor"]:                                               # everything but the anchor itself is ~0.9 m away
        assert traces[t]["m_depth"] is None and sorted(traces[t]["dist_margins"])[1] > 0.5
    for t, lo, hi in [(t, -0.035, -0.005) for t in c["near"]] + [(t, 0.005, 0.035) for t in c["far"]]:
        assert lo < traces[t]["dist_margins"][-1] < hi
    c = fc.case_by_name("selection")
    st, _, _, _, traces = fc.oracle_tracks(c, True)
    both = [(tr["m_depth"], tr["m_tri"]) for tr in traces if tr["m_depth"] is not None and tr["m_tri"] is not None
            and tr["m_depth"] <= 3.0 and tr["m_tri"] <= 3.0]
    assert sum(a < b for a, b in both) >= 5 and sum(a > b for a, b in both) >= 5
    assert (st == 1).sum() >= 5 and (st == 2).sum() >= 5
    c = fc.case_by_name("long_track")
    assert c["off"][c["long"] + 1] - c["off"][c["long"]] == 120 and np.bincount(c["img"][3:123]).tolist() == [3] * 40


def test_bucket_collisions_depend_on_the_container_order(monkeypatch):
    c = fc.case_by_name("bucket_collisions")
    for t in range(len(c["off"]) - 1):                                        # at least two images of every track share a bucket
        ids = c["img"][c["off"][t]:c["off"][t + 1]]
        B = fo.umap_bucket_count(len(ids))
        assert 5 <= len(ids) <= 12 and np.bincount(np.unique(ids) % B).max() >= 2
    want = fc.oracle_tracks(c, True)
    monkeypatch.setattr(fo, "umap_order", lambda keys, reserve_n: list(range(len(keys))))
    n_changed = 0
    for t in range(len(c["off"]) - 1):
        a, b = int(c["off"][t]), int(c["off"][t + 1])
        k = fo.fuse_track(c["img"][a:b], c["uv"][a:b], c["depth"], c["Rcw"], c["tcw"], c["intr"])[3]
        n_changed += not np.array_equal(k, want[3][a:b])
    assert n_changed >= 10, n_changed


def test_every_option_set_moves_tracks():
    c = fc.case_by_name("options")
    base = fc.oracle_tracks(c, True)[0]
    for o in c["option_sets"]:
        assert (fc.oracle_tracks(c, True, **o)[0] != base).sum() >= 3, o


def test_oracle_trace_changes_nothing_and_non_finite_pixels_have_no_depth():
    c = fc.case_by_name("selection")
    a, b = int(c["off"][3]), int(c["off"][4])
    args = (c["img"][a:b], c["uv"][a:b], c["depth"], c["Rcw"], c["tcw"], c["intr"])
    plain, traced = fo.fuse_track(*args), fo.fuse_track(*args, trace={})
    assert plain[0] == traced[0] and np.array_equal(plain[1], traced[1]) and plain[2] == traced[2] and np.array_equal(plain[3], traced[3])
    d = c["depth"][0]
    for u, v in ((np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (5.0, -np.inf)):
        assert fo.fetch_depth_bilinear(d, u, v) is None


def test_refusals_need_no_device(pkg):
    """The host checks of lvba_fuse_tracks / lvba_triangulate_tracks come before any device work, so they answer on a machine
    without a GPU: LVBA_ERR_ARG, the outputs as they were.  (tests/test_gpu_fusion_edges.py repeats them around good calls.)"""
    import ctypes as C
    L = pkg._lib
    lib = L.load()
    Rcw, tcw = fc.rig()
    R, t, intr = np.ascontiguousarray(Rcw).reshape(-1), np.ascontiguousarray(tcw).reshape(-1), np.ascontiguousarray(fc.INTR)
    img, uv, uv64 = np.zeros(6, np.int32), np.zeros((6, 2), np.float32), np.zeros((6, 2))

    def fuse(off, **o):
        out = (np.full(3, 0xAB, np.uint8), np.full(9, -7.5), np.full(3, -7.5), np.full(6, 0xCD, np.uint8))
        opts = L.FuseOpts()
        lib.lvba_fuse_default_opts(C.byref(opts))
        for k, v in o.items():
            setattr(opts, k, v)
        rc = lib.lvba_fuse_tracks(0, None, len(Rcw), R, t, intr, 3, np.array(off, np.int64), img.ctypes.data, uv.ctypes.data,
                                  C.byref(opts), out[0].ctypes.data, out[1], out[2], out[3].ctypes.data)
        return rc == L.ERR_ARG and (out[0] == 0xAB).all() and (out[1] == -7.5).all() and (out[2] == -7.5).all() and (out[3] == 0xCD).all()
    for off in ([0, 10, 3, 6], [0, 4, 2, 6], [1, 2, 4, 6]):
        assert fuse(off), off
        out = (np.full(9, -7.5), np.full(3, -7.5), np.full(3, -77, np.int32), np.full(3, 0xAB, np.uint8))
        rc = lib.lvba_triangulate_tracks(0, len(Rcw), 3, np.array(off, np.int64), img.ctypes.data, uv64.ctypes.data, R, t, intr, *out)
        assert rc == L.ERR_ARG and (out[0] == -7.5).all() and (out[2] == -77).all() and (out[3] == 0xAB).all(), off
    for o in (dict(obser_thr=0), dict(obser_thr=-3), dict(min_view_angle_deg=np.nan), dict(min_view_angle_deg=-0.5),
              dict(min_view_angle_deg=180.5), dict(min_view_angle_deg=-np.inf), dict(reproj_mean_thr_px=np.nan),
              dict(reproj_mean_thr_px=-1e-9)):
        assert fuse([0, 2, 4, 6], **o), o
