"""GPU tests of the scan-descriptor place recognition: the descriptors (lvba_place_descriptors), the search
(lvba_place_search, lvba_place_candidates) and pipeline.find_loop_closures(method="descriptor" / "both"), against the numpy
restatement (tests/place_oracle.py) on the shared fixtures (tests/place_cases.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import loop_cases as lc
import place_cases as pc
import place_oracle as po
import register_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("global-lvba_amd.register")


@pytest.fixture(scope="module")
def two_laps(pkg):
    sc = pkg.Scans(pc.clouds())
    yield sc
    sc.close()


def rows(got):
    return list(zip(*(got[k].tolist() for k in ("query", "submap", "ref", "shift", "distance", "yaw"))))


def test_descriptors_equal_the_oracle(pkg, reg):
    """The 24 frames of the two laps, an empty frame and a frame of 40 points: desc and ring_key bit for bit, twice; a sub-range
    is the slice; several workgroups per frame (a cloud of 40 000 points beside the small ones) merge to the same bytes."""
    clouds = pc.clouds() + [np.zeros((0, 3), np.float32), pc.clouds()[3][:40]]
    want = [po.descriptor(c, **pc.PLACE) for c in clouds]
    o = {k: pc.PLACE[k] for k in ("n_rings", "n_sectors", "min_range", "max_range", "z_offset")}
    with pkg.Scans(clouds) as sc:
        desc, key = reg.scan_descriptors(sc, **o)
        again = reg.scan_descriptors(sc, **o)
        part = reg.scan_descriptors(sc, frame_begin=5, n_frames=7, **o)
        tail = reg.scan_descriptors(sc, frame_begin=24, **pc.PLACE)
    assert desc.shape == (26, 20, 60) and key.shape == (26, 20)
    for f in range(26):
        assert desc[f].tobytes() == want[f][0].tobytes() and key[f].tobytes() == want[f][1].tobytes(), f
    assert not desc[24].any() and not key[24].any() and 0 < (desc[25] > 0).sum() <= 40 and (desc[:24] > 0).sum(axis=(1, 2)).min() > 300
    assert again[0].tobytes() == desc.tobytes() and again[1].tobytes() == key.tobytes()
    assert part[0].tobytes() == desc[5:12].tobytes() and part[1].tobytes() == key[5:12].tobytes()
    assert tail[0].tobytes() == desc[24:].tobytes()
    big = np.concatenate([c for c in pc.clouds()[:12]] + [pc.clouds()[0][:4000]])          # 40 000 points: three workgroups
    with pkg.Scans([pc.clouds()[1], big, np.zeros((0, 3), np.float32)]) as sc:
        d3, k3 = reg.scan_descriptors(sc, **o)
    wb = po.descriptor(big, **pc.PLACE)
    assert d3[1].tobytes() == wb[0].tobytes() and k3[1].tobytes() == wb[1].tobytes()
    assert d3[0].tobytes() == want[1][0].tobytes() and not d3[2].any()


@pytest.mark.parametrize("k", range(len(pc.search_cases())), ids=[c[0] for c in pc.search_cases()])
def test_search_equals_the_oracle(reg, k):
    name, desc, o, cap = pc.search_cases()[k]
    want, _ = pc.search_oracle(k)
    got = reg.place_search(desc, capacity=cap, **o)
    have = rows(got)
    n = len(want) if cap is None else min(cap, len(want))
    worst = max([abs(h[4] - w[4]) for h, w in zip(have, want)], default=0.0)
    print(f"{name}: {got['count']} candidates, {len(have)} fetched, largest |distance - oracle| {worst:.2e}")
    assert got["count"] == len(want) and len(have) == n
    assert [h[:4] for h in have] == [w[:4] for w in want[:n]]
    assert worst <= 1e-11
    assert [h[5] for h in have] == [po.yaw_of(h[3], o["n_sectors"]) for h in have]
    assert got["raw"].tobytes() == reg.place_search(desc, capacity=cap, **o)["raw"].tobytes()      # two calls, the same bytes


def test_capacity_and_bad_arguments(pkg, reg, two_laps):
    L = pkg._lib
    lib = L.load()
    name, desc, o, cap = next(c for c in pc.search_cases() if c[0] == "capacity")
    d = np.ascontiguousarray(desc)
    opts = L.PlaceOpts(**o)
    for cap in (0, 7):                                                          # nothing is written past the capacity
        buf = np.full(4 * (cap + 2), -7.0)
        n = C.c_int64()
        assert lib.lvba_place_search(0, len(d), d.ctypes.data, C.byref(opts), cap, buf.ctypes.data, C.byref(n)) == L.OK
        assert n.value > 7 and np.all(buf[4 * cap:] == -7.0)
    n = C.c_int64(-1)
    assert lib.lvba_place_search(0, 0, None, C.byref(opts), 0, None, C.byref(n)) == L.OK and n.value == 0       # n_frames = 0
    assert lib.lvba_place_descriptors(two_laps._h, 3, 0, C.byref(opts), None, None) == L.OK
    assert lib.lvba_place_search(0, len(d), d.ctypes.data, None, 0, None, C.byref(n)) == L.OK                    # NULL options

    def refused(rc):
        assert rc == L.ERR_ARG and lib.lvba_last_error()
    out = np.zeros(64, reg.PLACE_DTYPE)
    f4 = np.zeros((24, 20, 60), np.float32)
    lap = L.PlaceOpts(**po.options(**pc.PLACE))
    refused(lib.lvba_place_search(0, len(d), None, C.byref(opts), 0, None, C.byref(n)))
    refused(lib.lvba_place_search(0, len(d), d.ctypes.data, C.byref(opts), 4, None, C.byref(n)))
    refused(lib.lvba_place_search(0, len(d), d.ctypes.data, C.byref(opts), 0, None, None))
    refused(lib.lvba_place_search(0, -1, d.ctypes.data, C.byref(opts), 0, None, C.byref(n)))
    refused(lib.lvba_place_search(0, len(d), d.ctypes.data, C.byref(opts), -1, out.ctypes.data, C.byref(n)))
    refused(lib.lvba_place_descriptors(None, 0, 1, C.byref(lap), f4.ctypes.data, f4.ctypes.data))
    refused(lib.lvba_place_descriptors(two_laps._h, 0, 24, C.byref(lap), None, f4.ctypes.data))
    refused(lib.lvba_place_descriptors(two_laps._h, 0, 24, C.byref(lap), f4.ctypes.data, None))
    refused(lib.lvba_place_descriptors(two_laps._h, 0, -1, C.byref(lap), f4.ctypes.data, f4.ctypes.data))
    refused(lib.lvba_place_descriptors(two_laps._h, -1, 2, C.byref(lap), f4.ctypes.data, f4.ctypes.data))
    refused(lib.lvba_place_descriptors(two_laps._h, 20, 5, C.byref(lap), f4.ctypes.data, f4.ctypes.data))
    refused(lib.lvba_place_candidates(None, C.byref(lap), 0, None, C.byref(n)))
    refused(lib.lvba_place_candidates(two_laps._h, C.byref(lap), 0, None, None))
    refused(lib.lvba_place_candidates(two_laps._h, C.byref(lap), 4, None, C.byref(n)))
    refused(lib.lvba_place_candidates(two_laps._h, C.byref(lap), -1, out.ctypes.data, C.byref(n)))
    for bad in (dict(n_rings=0), dict(n_rings=33), dict(n_sectors=0), dict(n_sectors=129), dict(min_range=-0.1), dict(min_range=np.nan),
                dict(max_range=np.inf), dict(max_range=0.5, min_range=0.5), dict(z_offset=np.nan), dict(submap_size=0), dict(min_gap=-1),
                dict(n_key_candidates=0), dict(n_key_candidates=33), dict(max_per_frame=0), dict(max_per_frame=33), dict(query_stride=0),
                dict(max_distance=0.0), dict(max_distance=1.5), dict(max_distance=np.nan)):
        for call in (lambda kw: reg.place_candidates(two_laps, **kw), lambda kw: reg.scan_descriptors(two_laps, **kw)):
            with pytest.raises(L.LvbaError) as e:
                call(dict(pc.PLACE, **bad))
            assert e.value.code == L.ERR_ARG and str(e.value), bad
    small = pc.syn(7, 13)[0][:6].copy()
    for v in (np.nan, np.inf, -1.0):
        small[4, 2, 5] = v
        with pytest.raises(L.LvbaError) as e:
            reg.place_search(small, submap_size=1, min_gap=0)
        assert e.value.code == L.ERR_ARG and "frame 4" in str(e.value)
    with pytest.raises(TypeError):
        reg.place_candidates(two_laps, radius=2.0)
    with pytest.raises(TypeError):
        reg.place_search(small, n_keys=3)


def test_candidates_are_descriptors_then_search(reg, two_laps):
    desc, key = reg.scan_descriptors(two_laps, **pc.PLACE)
    assert desc.tobytes() == pc.descriptors()[0].tobytes() and key.tobytes() == pc.descriptors()[1].tobytes()
    a = reg.place_candidates(two_laps, **pc.PLACE)
    b = reg.place_search(desc, **pc.PLACE)
    assert a["count"] == b["count"] == 24 and a["raw"].tobytes() == b["raw"].tobytes()
    assert a["raw"].tobytes() == reg.place_candidates(two_laps, **pc.PLACE)["raw"].tobytes()
    want, _ = pc.candidates()
    assert [r[:4] for r in rows(a)] == [w[:4] for w in want]
    part = reg.place_candidates(two_laps, capacity=5, **pc.PLACE)
    assert part["count"] == 24 and part["raw"].tobytes() == a["raw"][:5].tobytes()


def relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_find_loop_closures_by_descriptor(pkg, two_laps):
    """At the drifted poses -- lap B 9 m and 10 degrees off, where the pose-based search finds nothing -- method="descriptor"
    finds every revisit, starts every registration from poses[ref] o Rz(yaw), and status, inliers, acceptance and priors are the
    oracle's from the same start."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    x = pc.drifted()
    shared = {k: pc.PLACE[k] for k in ("submap_size", "min_gap", "max_per_frame")}
    place = {k: v for k, v in pc.PLACE.items() if k not in shared}
    kw = dict(voxel_size=lc.VS, **shared, **pc.ACCEPT, **pc.REG)
    priors, report = pl.find_loop_closures(two_laps, x, method="descriptor", place=place, **kw)
    want, _ = pc.candidates()
    assert [(r["query"], r["submap"], r["ref"], r["shift"]) for r in report] == [w[:4] for w in want]
    assert all(r["method"] == "descriptor" and r["distance_kind"] == "descriptor" for r in report)
    assert max(abs(r["distance"] - w[4]) for r, w in zip(report, want)) <= 1e-11 and [r["yaw"] for r in report] == [w[5] for w in want]
    accepted = []
    for r in report:
        if r["query"] < 12:
            continue
        start, o, (ok, why) = pc.oracle_register(r["query"], r["submap"], r["ref"], r["shift"])
        assert np.abs(r["start"] - start).max() <= 1e-15 and np.abs(r["start"] - po.start_pose(x[r["ref"]], r["yaw"])).max() <= 1e-15
        print(f"query {r['query']}: status {r['status_name']}, iterations {r['iterations']} / {o['iterations']}, inliers {r['inliers']} / "
              f"{o['inliers']}, rmse {r['rmse']:.5f} / {o['rmse']:.5f}, |pose - oracle| {np.abs(r['pose'] - o['pose']).max():.2e}, {r['accepted']} {r['reason']}")
        assert r["status"] == o["status"] and r["iterations"] == o["iterations"] and r["inliers"] == o["inliers"]
        assert np.abs(r["pose"] - o["pose"]).max() <= 1e-7
        assert (r["accepted"], r["reason"]) == (ok, why)
        if ok:
            accepted.append((r, o))
    assert len(accepted) >= 8
    mine = [p for p in priors if p.j >= 12]
    assert len(mine) == len(accepted)
    for p, (r, o) in zip(mine, accepted):
        q = pl.registration_prior(r["ref"], r["query"], x[r["ref"]], o["pose"], o["information"], o["rmse"], o["status"])
        assert (p.i, p.j) == (r["ref"], r["query"]) and relmax(p.meas[:], q.meas[:]) <= 1e-7 and relmax(p.sqrt_info[:], q.sqrt_info[:]) <= 1e-7
    # the registered pose, relative to ref, is the true relative pose: the prior closes the 9 m
    P = pc.truth()
    for r, _ in accepted:
        Rr, Rq = x[r["ref"], :9].reshape(3, 3), P[r["ref"], :9].reshape(3, 3)
        got = Rr.T @ (r["pose"][9:] - x[r["ref"], 9:])
        true = Rq.T @ (P[r["query"], 9:] - P[r["ref"], 9:])
        assert np.linalg.norm(got - true) < 0.02 and np.linalg.norm(r["pose"][9:] - x[r["query"], 9:]) > 5.0
    # the pose-based search at the same poses: nothing
    assert pl.find_loop_closures(two_laps, x, method="pose", radius=pc.POSE_RADIUS, **kw) == ([], [])
    with pytest.raises(ValueError):
        pl.find_loop_closures(two_laps, x, method="appearance", **kw)
    with pytest.raises(TypeError):
        pl.find_loop_closures(two_laps, x, method="descriptor", place=dict(min_gap=3), **kw)


def test_pose_method_is_unchanged_and_both_is_a_union(pkg):
    """On loop_cases' drifted fixture method="pose" (the default) reports the four candidates of DESIGN.md §10d with the oracle's
    verdicts; "both" holds every pair once, the pairs both found with the pose-based start."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    x = lc.drifted()
    kw = dict(submap_size=lc.S, voxel_size=lc.VS, radius=lc.RADIUS, min_gap=lc.MIN_GAP, **lc.ACCEPT, **lc.OPTS)
    place = {k: pc.PLACE[k] for k in ("n_rings", "n_sectors", "max_range", "min_range", "z_offset", "n_key_candidates")}
    with pkg.Scans([c[:, :3] for c in lc.scans()["clouds"]]) as sc:
        priors, report = pl.find_loop_closures(sc, x, **kw)
        named = pl.find_loop_closures(sc, x, method="pose", **kw)
        _, desc = pl.find_loop_closures(sc, x, method="descriptor", place=place, **kw)
        _, both = pl.find_loop_closures(sc, x, method="both", place=place, **kw)
    cand = lc.candidates("drifted")
    assert len(cand) == 4 and [(r["query"], r["submap"], r["ref"], r["distance"]) for r in report] == cand
    want = [lc.oracle_accept("drifted", q, w) for q, w, _, _ in cand]
    assert [(r["accepted"], r["reason"]) for r in report] == [(ok, why) for ok, why, _ in want]
    for r, (_, _, o) in zip(report, want):
        assert r["method"] == "pose" and r["distance_kind"] == "metres" and r["shift"] is None and r["yaw"] is None
        assert r["start"].tobytes() == x[r["query"]].tobytes() and r["iterations"] == o["iterations"] and r["inliers"] == o["inliers"]
        assert np.abs(r["pose"] - o["pose"]).max() <= 1e-7
    assert len(priors) == sum(ok for ok, _, _ in want)
    for a, b in zip(report, named[1]):
        assert a["pose"].tobytes() == b["pose"].tobytes() and a["information"].tobytes() == b["information"].tobytes()
    assert [(p.i, p.j) for p in priors] == [(p.i, p.j) for p in named[0]]
    pairs = [(r["query"], r["submap"]) for r in both]
    pose_pairs, desc_pairs = {(c[0], c[1]) for c in cand}, {(r["query"], r["submap"]) for r in desc}
    assert pairs == sorted(set(pairs)) and set(pairs) == pose_pairs | desc_pairs
    print(f"pose {sorted(pose_pairs)}, descriptor {sorted(desc_pairs)}")
    for r in both:
        key = (r["query"], r["submap"])
        assert r["method"] == ("both" if key in pose_pairs & desc_pairs else "pose" if key in pose_pairs else "descriptor")
        if key in pose_pairs:
            assert r["start"].tobytes() == x[r["query"]].tobytes() and r["distance_kind"] == "metres"
            assert r["pose"].tobytes() == next(a for a in report if (a["query"], a["submap"]) == key)["pose"].tobytes()
