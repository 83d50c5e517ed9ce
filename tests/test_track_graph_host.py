"""CPU tests of the device track builder (include/lvba_hip.h "feature tracks on the device"): the device header
compiled for the host behind a stand-alone driver against the host mirror (pipeline.match_graph / match_components / bfs_order)
bit for bit on every case of tests/track_graph_cases.py, the same driver under the address and undefined-behaviour sanitizers, the
info struct's size, and the wiring of device_tracks through the pipeline on a stub TrackGraph backed by the host functions."""
import ctypes
import importlib
import os
import sqlite3
import subprocess

import numpy as np
import pytest

import track_graph_cases as tc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "track_graph_check.cpp")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("track_graph"), "track_graph_check", "-O2")


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("track_graph_san"), "track_graph_check_san", "-O1", "-g", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all")


def run_driver(exe, tmp_path, name, thr, lanes, attempts):
    """the driver's output as a dict, with orders = {attempt: (sel, obs_off, obs_img, obs_kp)}"""
    c = tc.case(name)
    kp_off = np.concatenate([[0], np.cumsum(c["n_keypoints"])]).astype(np.int64)
    match_off = np.concatenate([[0], np.cumsum([len(m) for m in c["matches"]])]).astype(np.int64)
    flat = np.concatenate(c["matches"]).reshape(-1) if c["matches"] else np.zeros(0, np.int64)
    words = np.concatenate([[len(c["n_keypoints"])], kp_off, [len(c["pairs"])], np.asarray(c["pairs"], np.int64).reshape(-1), match_off, flat,
                            [thr, lanes, len(attempts)], attempts]).astype(np.int64)
    fin, fout = tmp_path / f"{name}_{thr}_{lanes}.in", tmp_path / f"{name}_{thr}_{lanes}.out"
    words.tofile(fin)
    done = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert done.returncode == 0, (name, thr, lanes, done.returncode, done.stderr[-2000:])
    w = np.fromfile(fout, np.int64)
    at = [0]

    def take(n):
        at[0] += int(n)
        return w[at[0] - int(n):at[0]]

    keys = ("n_nodes", "n_edges", "n_skipped", "n_components_all", "n_components", "n_observations", "largest_component", "rounds")
    out = dict(info=dict(zip(keys, take(8).tolist())))
    N, nc, no = int(kp_off[-1]), out["info"]["n_components"], out["info"]["n_observations"]
    out["adj_off"] = take(N + 1)
    out["adj"] = take(2 * out["info"]["n_edges"])
    out["comp_off"], out["mem_img"], out["mem_kp"], out["comp_images"] = take(nc + 1), take(no), take(no), take(nc)
    out["orders"] = {}
    for a in attempts:
        sel = take(take(1)[0])
        off = take(len(sel) + 1)
        out["orders"][a] = (sel, off, take(off[-1]), take(off[-1]))
    assert at[0] == len(w)
    return out


def check_against_the_mirror(got, name, thr, attempts):
    want = tc.expected(name, thr)
    rounds = got["info"].pop("rounds")
    assert got["info"] == want["info"], (name, thr)
    assert 0 <= rounds <= 64 and (rounds >= 1) == (want["info"]["n_edges"] > 0)
    for key in ("adj_off", "adj", "comp_off", "mem_img", "mem_kp", "comp_images"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name} {thr} {key}")
    for a in attempts:
        sel, off, img, kp = got["orders"][a]
        assert sel.tolist() == tc.with_more_than(name, thr, a)
        for x, y in zip((off, img, kp), tc.expected_orders(name, thr, a, sel)):
            np.testing.assert_array_equal(x, y, err_msg=f"{name} {thr} attempt {a}")


def test_cases_hold_what_they_are_for():
    """the hub's neighbour list crosses the batch of 64 twice with its planted duplicates in place, the chain is one component, the
    giant is there beside its tracks, every threshold has its two edge components"""
    adj, _ = tc.graph("hub")
    hub = adj[0][1]
    assert len(hub) == tc.HUB_FAN + len(tc.HUB_DUPLICATES) > 128
    for k, (p, q) in tc.HUB_DUPLICATES.items():
        assert hub[p] == hub[q] == (1, k)
    places = tc.HUB_DUPLICATES.values()
    assert any(p // 8 == q // 8 for p, q in places) and any(p // 64 == q // 64 and p // 8 != q // 8 for p, q in places)
    assert any(p // 64 != q // 64 for p, q in places)
    assert [len(m) for m in tc.expected("chain", 3)["comps"]] == [300]
    sizes = sorted(len(m) for m in tc.expected("giant", 3)["comps"])
    assert sizes[-1] == 5000 and len(sizes) == 1001 and 3 <= sizes[0] and sizes[-2] <= 6
    assert tc.expected("random", 1)["info"]["n_skipped"] > 0 and any(len(set(v)) < len(v) for a in tc.graph("random")[0] for v in a.values())
    shapes = {(len(m), len({i for i, _ in m})) for m in tc.expected("thresholds", 1)["comps"]}
    assert {(6, 2), (5, 4), (2, 2), (3, 3), (4, 4), (5, 5)} <= shapes
    for thr in tc.THRESHOLDS:
        kept = {(len(m), len({i for i, _ in m})) for m in tc.expected("thresholds", thr)["comps"]}
        assert kept == {s for s in shapes if min(s) >= thr}
    for name in tc.NAMES[6:]:
        assert tc.expected(name, 1)["info"]["n_nodes"] == 0


@pytest.mark.parametrize("name", tc.NAMES)
def test_device_header_on_the_host_equals_the_mirror(driver, tmp_path, name):
    """half-edge placement, adjacency, labels under two schedules, members, the two checks and the orders of every attempt the GPU
    tests walk, for all four thresholds; batches of 8 lanes (the library's), and of 64 at the reference's threshold"""
    for thr, lanes in [(t, 8) for t in tc.THRESHOLDS] + [(3, 64)]:
        attempts = tc.attempts_of(name, thr)
        check_against_the_mirror(run_driver(driver, tmp_path, name, thr, lanes, attempts), name, thr, attempts)


@pytest.mark.parametrize("name", tc.EVERY_ATTEMPT)
def test_driver_under_the_sanitizers(sanitized_driver, tmp_path, name):
    """every BFS segment is a heap block of exactly the component's size: an overrun, a read past the adjacency or an overflow stops
    the program"""
    for thr, lanes in ((1, 8), (3, 8), (3, 64)):
        attempts = tc.attempts_of(name, thr)
        check_against_the_mirror(run_driver(sanitized_driver, tmp_path, name, thr, lanes, attempts), name, thr, attempts)


def test_info_struct_has_the_size_the_c_compiler_gives_it(pkg):
    assert ctypes.sizeof(pkg._lib.TrackGraphInfo) == 64            # against the header: tests/test_abi.py, every struct at once
    assert {"lvba_trackgraph_create", "lvba_trackgraph_components", "lvba_trackgraph_orders", "lvba_trackgraph_destroy"} <= set(pkg._lib.SYMBOLS)


# ---- the wiring of device_tracks, on a TrackGraph backed by the host functions -----------------------------------------------
class HostTrackGraph:
    """trackgraph.TrackGraph's interface over pipeline.match_components / bfs_order"""
    made = []

    def __init__(self, keypoints, pairs, matches, obser_thr=3, device=0):
        pl = tc.pipeline()
        self.keypoints = keypoints
        self.adj, self.comps = pl.match_components([len(k) for k in keypoints], pairs, matches, obser_thr)
        self.calls = []
        HostTrackGraph.made.append(self)

    def components(self):
        flat = [ob for m in self.comps for ob in m]
        return (np.concatenate([[0], np.cumsum([len(m) for m in self.comps])]).astype(np.int64), np.array([i for i, _ in flat], np.int32),
                np.array([k for _, k in flat], np.int32), np.array([len({i for i, _ in m}) for m in self.comps], np.int32))

    def orders(self, comp=None, attempt=0, uv=False):
        comp = list(range(len(self.comps))) if comp is None else [int(c) for c in comp]
        assert all(a < b for a, b in zip(comp, comp[1:])) and uv
        self.calls.append((comp, attempt))
        orders = [tc.pipeline().bfs_order(self.adj, self.comps[c][attempt]) for c in comp]
        flat = [ob for o in orders for ob in o]
        return (np.concatenate([[0], np.cumsum([len(o) for o in orders])]).astype(np.int64), np.array([i for i, _ in flat], np.int32),
                np.array([k for _, k in flat], np.int32), np.array([self.keypoints[i][k][:2] for i, k in flat], np.float32).reshape(-1, 2))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True


def fuse_stubs():
    """a fusion that never accepts, one that accepts a component on its second attempt, one that always accepts; what they return
    depends on what they are handed, so that a track in the wrong place or order shows"""
    seen = {}

    def answer(off, img, uv, ok):
        n = len(off) - 1
        first = off[:-1]
        X = np.stack([np.add.reduceat(uv[:, 0].astype(np.float64), first) if n else np.zeros(0), img[first].astype(np.float64),
                      np.diff(off).astype(np.float64)], 1) if n else np.zeros((0, 3))
        return (np.where(ok, 1 + (img[first] % 2), 0).astype(np.uint8), X, X[:, 0] / np.maximum(X[:, 2], 1), (uv[:, 0] > 320).astype(np.uint8))

    def never(off, img, uv):
        return answer(off, img, uv, np.zeros(len(off) - 1, bool))

    def second(off, img, uv):
        members = [frozenset(zip(img[a:b].tolist(), np.round(uv[a:b, 0], 3).tolist())) for a, b in zip(off[:-1], off[1:])]
        ok = np.array([m in seen.get(id(second), set()) for m in members], bool)
        seen.setdefault(id(second), set()).update(members)
        return answer(off, img, uv, ok)

    def always(off, img, uv):
        return answer(off, img, uv, np.ones(len(off) - 1, bool))

    return dict(never=never, second=second, always=always), seen


@pytest.mark.parametrize("name", ("random", "thresholds", "four_views", "no_pairs"))
def test_track_loop_on_device_orders_equals_the_host_loop(monkeypatch, name):
    pl = tc.pipeline()
    tg = importlib.import_module("global-lvba_amd.trackgraph")
    monkeypatch.setattr(tg, "TrackGraph", HostTrackGraph)
    c = tc.case(name)
    for thr in (2, 3):
        for kind in ("never", "second", "always"):
            stubs, seen = fuse_stubs()
            want = pl.build_tracks_and_fuse(c["keypoints"], c["pairs"], c["matches"], stubs[kind], thr)
            seen.clear()
            HostTrackGraph.made.clear()
            got = pl.build_tracks_and_fuse(c["keypoints"], c["pairs"], c["matches"], stubs[kind], thr, device_tracks=True)
            assert got.keys() == want.keys()
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name} {thr} {kind} {key}")
                assert got[key].dtype == want[key].dtype, (name, kind, key)
            (g,) = HostTrackGraph.made                                          # one graph, closed, one orders call per round
            assert g.closed and [a for _, a in g.calls] == list(range(len(g.calls)))
            if kind == "always" and g.comps:
                assert len(g.calls) == 1 and got["attempts"].max() == 0
            if kind == "second" and g.comps:
                assert got["attempts"].tolist() == [1] * len(g.comps)
            if kind == "never" and g.comps:
                assert len(g.calls) == max(len(m) for m in g.comps) and len(got["X"]) == 0


def test_device_tracks_is_handed_down(monkeypatch, tmp_path):
    """run_dataset -> run_full_pipeline -> run_visual_ba_with_lidar_assist -> build_tracks_and_fuse: the keyword arrives when it is
    set and is absent (the default, False) when it is not"""
    pl = tc.pipeline()
    ds = importlib.import_module("global-lvba_amd.dataset")
    calls = []
    empty = pl.build_tracks_and_fuse([], [], [], None)

    # the visual stage hands it to the track loop
    monkeypatch.setattr(pl, "build_tracks_and_fuse", lambda *a, **k: calls.append(k) or empty)
    pose = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64), (2, 1))
    args = (None, pose, pose, [0.0, 1.0], [0.0, 1.0], pose, np.eye(3), np.zeros(3), np.ones(8), 8, 8, [np.zeros((2, 2))] * 2, [], [])
    for flag in (True, False):
        out = pl.run_visual_ba_with_lidar_assist(*args, depth=object(), **({"device_tracks": True} if flag else {}))
        assert out["termination"] == "NO_TRACKS" and calls[-1].get("device_tracks", False) is flag

    # the full pipeline hands it to the visual stage
    class NoScans:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    monkeypatch.setattr(pl, "Scans", NoScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append(k) or {})
    full = ([], pose, [0.0, 1.0], [0.0, 1.0], pose, np.eye(3), np.zeros(3), np.ones(8), 8, 8, [np.zeros((2, 2))] * 2, [], [])
    pl.run_full_pipeline(*full, enable_lidar_ba=False, device_tracks=True)
    assert calls[-1]["device_tracks"] is True
    pl.run_full_pipeline(*full, enable_lidar_ba=False)
    assert "device_tracks" not in calls[-1]

    # the dataset entry hands it to the full pipeline
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    stamps = (0.5, 1.5)
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
    monkeypatch.setattr(pl, "run_full_pipeline", lambda *a, **k: calls.append(k) or dict(poses=np.tile(np.eye(3, 4).reshape(-1), (2, 1))))
    where = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    pl.run_dataset(*where, device_tracks=True)
    assert calls[-1]["device_tracks"] is True
    pl.run_dataset(*where)
    assert "device_tracks" not in calls[-1]
