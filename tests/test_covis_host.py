"""CPU tests of the co-visibility pair selection (include/lvba_hip.h "which image pairs to match"): the numpy oracle
against the rule as plain loops, the device header compiled for the host against the oracle bit for bit, the fixture's
conditions (margins, branches, the tie at the cap), the options struct's size, and the claim -- with the occlusion test no pair
that shares nothing is selected and no pair that shares much is missed, without it pairs across the partition come in."""
import ctypes
import importlib
import json
import sqlite3

import numpy as np
import pytest

import covis_cases as cc
import covis_oracle as co
import match_cases as mc
from host_build import build_check

# The largest number of planted points (of cc.N_PLANTED) that a pair NOT selected at the defaults shares is 63, measured on this
# fixture by the oracle at 160 x 128 with the 16 x 12 grid: no pair sharing this many may be missed.
T_SHARED = 64


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/covis_device.h compiled for the host, without contraction (tests/covis_check.cpp)"""
    lib = ctypes.CDLL(build_check("covis_check", tmp_path_factory.mktemp("emul_covis")))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.emul_samples.argtypes = [I, I, I, I, I, I, P, P, P, P, P, P]
    lib.emul_counts.argtypes = [I, I, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.emul_select.argtypes = [I, P, P, P, P, P, P, P]
    lib.emul_samples.restype = lib.emul_counts.restype = None
    lib.emul_select.restype = ctypes.c_int64
    return lib


def ptr(x):
    return x.ctypes.data


def rule_arrays(**kw):
    o = dict(co.DEFAULTS, **kw)
    return (np.array([o["occlusion"], o["both_ways"], o["max_per_image"], o["min_shared"]], np.int32),
            np.array([o["min_overlap"], o["occlusion_rel"], o["occlusion_abs"]], np.float64))


def host_samples(emul, r, grid, M):
    gx, gy = cc.GRIDS[grid]
    world, ring = np.zeros((M, gx * gy, 3)), np.zeros((M, gx * gy), np.int32)
    emul.emul_samples(M, r["W"], r["H"], gx, gy, co.DEFAULTS["search_radius"], ptr(r["depth"]), ptr(r["Rcw"]), ptr(r["tcw"]), ptr(r["intr"]),
                      ptr(world), ptr(ring))
    return world, ring


def host_counts(emul, r, world, M, occlusion):
    G = world.shape[1]
    fate, n, c = np.zeros((M, M, G), np.int32), np.zeros(M, np.int32), np.zeros((M, M), np.int32)
    rule, bounds = rule_arrays(occlusion=occlusion)
    emul.emul_counts(M, r["W"], r["H"], G, ptr(r["depth"]), ptr(r["Rcw"]), ptr(r["tcw"]), ptr(r["intr"]), ptr(rule), ptr(bounds),
                     ptr(np.ascontiguousarray(world)), ptr(fate), ptr(n), ptr(c))
    return fate, n, c


def host_select(emul, n, c, **kw):
    M = len(n)
    cap = max(M * (M - 1) // 2, 1)
    pairs, score, shared = np.zeros((cap, 2), np.int32), np.zeros(cap), np.zeros((cap, 2), np.int32)
    rule, bounds = rule_arrays(**kw)
    m = emul.emul_select(M, ptr(rule), ptr(bounds), ptr(np.ascontiguousarray(n, np.int32)), ptr(np.ascontiguousarray(c, np.int32)),
                         ptr(pairs), ptr(score), ptr(shared))
    return pairs[:m], score[:m], shared[:m]


def test_oracle_equals_the_rule_as_loops():
    """the 37 x 29 images, the 7 x 5 grid: samples, counts with and without the occlusion test, and the selection"""
    r = cc.room(1)
    world, _ = cc.lifted(1, 1)
    np.testing.assert_array_equal(co.loops_samples(r["depth"], r["intr"], r["Rcw"], r["tcw"], **cc.grid_opts(1)), world)
    for occlusion in (0, 1):
        _, _, n, c = cc.judged(1, 1, occlusion)
        ln, lc = co.loops_counts(r["depth"], r["intr"], r["Rcw"], r["tcw"], world, occlusion=occlusion)
        np.testing.assert_array_equal(ln, n)
        np.testing.assert_array_equal(lc, c)
    for kw in cc.OPTION_SETS:
        _, _, n, c = cc.judged(1, 1, dict(co.DEFAULTS, **kw)["occlusion"])
        pairs, score, shared = co.select(n, c, **kw)
        want = co.loops_select(n, c, **kw)
        assert [tuple(p) for p in pairs.tolist()] == [w[:2] for w in want], kw
        assert score.tolist() == [w[2] for w in want] and shared.tolist() == [list(w[3:]) for w in want], kw


def test_device_header_on_the_host_equals_the_oracle(emul):
    """samples, fates, counts and the selection, bit for bit, on every shape the GPU tests use"""
    for size in range(len(cc.SIZES)):
        r = cc.room(size)
        for grid in range(len(cc.GRIDS)):
            for M in cc.M_VALUES:
                world, ring = cc.lifted(size, grid, M)
                hw, hr = host_samples(emul, r, grid, M)
                np.testing.assert_array_equal(hw, world)
                np.testing.assert_array_equal(hr, ring)
                for occlusion in (0, 1):
                    fate, _, n, c = cc.judged(size, grid, occlusion, M)
                    hf, hn, hc = host_counts(emul, r, world, M, occlusion)
                    np.testing.assert_array_equal(hf, fate)
                    np.testing.assert_array_equal(hn, n)
                    np.testing.assert_array_equal(hc, c)
                for kw in cc.OPTION_SETS:
                    _, _, n, c = cc.judged(size, grid, dict(co.DEFAULTS, **kw)["occlusion"], M)
                    for got, want in zip(host_select(emul, n, c, **kw), co.select(n, c, **kw)):
                        np.testing.assert_array_equal(got, want, err_msg=f"{size} {grid} {M} {kw}")


def test_fixture_conditions():
    assert cc.check_margins() >= mc.MIN_MARGIN
    for size in range(len(cc.SIZES)):
        world, ring = cc.lifted(size, 0)
        assert (ring >= 1).any() and (ring < 0).any()                          # a cell resolved on a ring, a cell with no point
        assert (ring[cc.HOLES] >= 1).any() and (ring[cc.HOLES] < 0).any() and (ring[cc.EMPTY] < 0).all()
        assert (ring[:cc.N_CAMERAS] == 0).all()
        fate, _, n, _ = cc.judged(size, 0, 1)
        for kind in (co.BEHIND, co.OUTSIDE, co.HIDDEN, co.SEEN_HOLE, co.SEEN):
            assert (fate == kind).any(), kind
        assert n[cc.EMPTY] == 0 and 0 < n[cc.HOLES] < world.shape[1] and (n[:cc.N_CAMERAS] == world.shape[1]).all()
        assert not (cc.judged(size, 0, 0)[0] == co.HIDDEN).any()
    # the twin ties with camera 0 in every other image's ranking: a tie exactly at the cap, for both caps the tests use
    _, _, n, c = cc.judged(0, 0, 1)
    score, _, eligible = co.pair_terms(n, c)
    for K in (1, 3):
        tied = [i for i in range(cc.N_IMAGES) if len(p := co.ranked_partners(score, eligible, i)) > K and score[i, p[K - 1]] == score[i, p[K]]]
        assert tied, K
    # the option sets do select different things
    sets = [frozenset(map(tuple, cc.selected(0, 0, **kw)[0].tolist())) for kw in cc.OPTION_SETS]
    assert len(set(sets)) == len(sets) and all(sets)


def test_occlusion_keeps_out_the_pairs_that_share_nothing():
    """against the planted surface points whose visibility the fixture ray-casts, over the 18 cameras at min_overlap = 0.1"""
    shared = cc.shared_planted(0)
    N = cc.N_CAMERAS
    every = {(i, j) for i in range(N) for j in range(i + 1, N)}

    def chosen(occlusion):
        _, _, n, c = cc.judged(0, 0, occlusion)
        return set(map(tuple, co.select(n[:N], c[:N, :N], occlusion=occlusion, min_overlap=0.1)[0].tolist()))

    on, off = chosen(1), chosen(0)
    print(f"pairs {len(every)}, selected {len(on)} with / {len(off)} without the occlusion test; sharing nothing: "
          f"{sum(shared[p] == 0 for p in on)} / {sum(shared[p] == 0 for p in off)} of {sum(shared[p] == 0 for p in every)}; "
          f"largest share missed: {max(shared[p] for p in every - on)} / {max(shared[p] for p in every - off)}")
    assert not [p for p in on if shared[p] == 0]                               # no selected pair shares nothing
    assert not [p for p in every - on if shared[p] >= T_SHARED]                # no pair that shares much is missed
    assert [p for p in off if shared[p] == 0]                                  # without the test, pairs across the partition come in
    assert on < off and len(on) < len(every) // 4


def test_run_dataset_wires_the_pair_selection(tmp_path, monkeypatch):
    """run_dataset(pair_selection=...) on a two-image directory with run_full_pipeline and the matcher stubbed: refused for "db" and
    "descriptors" before anything is read, handed on as match_select for "guided" and "depth", an inner match_fn that takes the
    selected pairs (all pairs when none are given), and pair_selection.json in out_dir."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    for matching in ("db", "descriptors"):
        with pytest.raises(ValueError, match="pair_selection"):
            pl.run_dataset(str(tmp_path / "nowhere"), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3), matching=matching, pair_selection=True)
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    stamps = (0.5, 1.5, 2.5)
    for t in stamps:
        ds.save_pcd(str(tmp_path / "all_pcd_body" / f"{t}.pcd"), rng.normal(size=(10, 4)).astype(np.float32))
        (tmp_path / "all_image" / f"{t}.png").write_bytes(b"")
    poses = "".join(f"{t} {k} 0 0 0 0 0 1\n" for k, t in enumerate(stamps))
    (tmp_path / "all_pcd_body" / "lidar_poses.txt").write_text(poses)
    (tmp_path / "all_image" / "image_poses.txt").write_text(poses)
    con = sqlite3.connect(str(tmp_path / "db.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    kp = rng.uniform(0, 500, (6, 4)).astype(np.float32)
    for iid, t in enumerate(stamps):
        con.execute("INSERT INTO images VALUES (?, ?)", (iid + 1, f"{t:.6f}.png"))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (iid + 1, 6, 4, kp.tobytes()))
    con.commit(); con.close()
    report = dict(n_images=3, all_pairs=3, selected=1, covisible=1, empty_images=[])
    calls, matched = [], []

    def full_pipeline(*a, **k):
        calls.append(k)
        return dict(poses=np.tile(np.eye(3, 4).reshape(-1), (3, 1)), **({"pair_selection": report} if k.get("match_select") else {}))

    def match_image_pairs(descs, pairs, **k):
        matched.append((list(pairs), k.get("depth")))
        return [np.array([[0, 1]], np.int32) if p == (0, 2) else np.zeros((0, 2), np.int32) for p in pairs]

    monkeypatch.setattr(pl, "run_full_pipeline", full_pipeline)
    monkeypatch.setattr(pl, "match_image_pairs", match_image_pairs)
    monkeypatch.setattr(ds, "load_colmap_descriptors", lambda *a, **k: [np.zeros((6, 128), np.uint8)] * 3)
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    for matching, sel in (("guided", True), ("depth", dict(sequential=1, min_overlap=0.2))):
        out_dir = tmp_path / f"out_{matching}"
        out = pl.run_dataset(*args, matching=matching, pair_selection=sel, out_dir=str(out_dir))
        k = calls[-1]
        assert k["match_select"] is sel and callable(k["match_fn"]) and k.get("match_depth", False) == (matching == "depth")
        assert out["pair_selection"] == report == json.load(open(out_dir / "pair_selection.json"))
        cam = np.tile(np.eye(3, 4).reshape(-1), (3, 1))
        pairs, ms = k["match_fn"](cam, pairs=[(0, 2), (1, 2)], depth="D")     # the selected pairs, and those alone
        assert matched[-1] == ([(0, 2), (1, 2)], "D") and pairs == [(0, 2)] and len(ms) == 1
        pairs, ms = k["match_fn"](cam)                                        # no selection handed in: all pairs
        assert matched[-1] == ([(0, 1), (0, 2), (1, 2)], None) and pairs == [(0, 2)] and len(ms) == 1
    pl.run_dataset(*args, matching="guided", out_dir=str(tmp_path / "plain"))                 # off by default
    assert "match_select" not in calls[-1] and not (tmp_path / "plain" / "pair_selection.json").exists()


def test_match_select_needs_match_fn():
    pl = importlib.import_module("global-lvba_amd.pipeline")
    a = ([], np.zeros((0, 12)), [], [], np.zeros((0, 12)), np.eye(3), np.zeros(3), np.ones(8), 4, 4, [], [], [])
    with pytest.raises(ValueError, match="match_select"):
        pl.run_full_pipeline(*a, match_select=True)
    with pytest.raises(ValueError, match="match_select"):
        pl.run_full_pipeline(*a, match_select=True, match_fn=lambda *x, **k: ([], []), enable_visual_ba=False)
