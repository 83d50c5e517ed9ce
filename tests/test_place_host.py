"""CPU tests of the scan-descriptor place recognition: the device header (csrc/place_device.h) compiled for the host against the
numpy restatement (tests/place_oracle.py), the conditions on the shared fixtures (tests/place_cases.py) and the
struct layouts."""
import ctypes
import importlib

import numpy as np
import pytest

from host_build import build_check

import place_cases as pc
import place_oracle as po
import register_oracle as ro


class EmulOpts(ctypes.Structure):
    _fields_ = [("n_rings", ctypes.c_int32), ("n_sectors", ctypes.c_int32), ("min_range", ctypes.c_double), ("max_range", ctypes.c_double),
                ("z_offset", ctypes.c_double), ("submap_size", ctypes.c_int32), ("min_gap", ctypes.c_int32),
                ("n_key_candidates", ctypes.c_int32), ("max_per_frame", ctypes.c_int32), ("query_stride", ctypes.c_int32),
                ("pad", ctypes.c_int32), ("max_distance", ctypes.c_double)]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("place_check", tmp_path_factory.mktemp("emul_place")))
    f32, f64, i32 = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.float64, np.int32))
    lib.emul_descriptor.argtypes = [ctypes.c_int64, f32, ctypes.POINTER(EmulOpts), i32, f32, f32, f32]
    lib.emul_descriptor.restype = None
    lib.emul_search.argtypes = [ctypes.c_int, f32, ctypes.POINTER(EmulOpts), ctypes.c_int64, i32, i32, i32, i32, f64, f64]
    lib.emul_search.restype = ctypes.c_int64
    return lib


def host_descriptor(emul, cloud, **kw):
    o = EmulOpts(**po.options(**kw))
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    cell, h = np.zeros(max(len(xyz), 1), np.int32), np.zeros(max(len(xyz), 1), np.float32)
    D, key = np.zeros((o.n_rings, o.n_sectors), np.float32), np.zeros(o.n_rings, np.float32)
    emul.emul_descriptor(len(xyz), xyz if len(xyz) else np.zeros((1, 3), np.float32), ctypes.byref(o), cell, h, D, key)
    return cell[:len(xyz)], h[:len(xyz)], D, key


def host_search(emul, desc, capacity=None, **kw):
    o = EmulOpts(**po.options(**kw))
    d = np.ascontiguousarray(desc, np.float32)
    cap = max(1, len(d) * o.max_per_frame) if capacity is None else capacity
    q, w, r, s = (np.zeros(max(cap, 1), np.int32) for _ in range(4))
    dist, yaw = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
    n = emul.emul_search(len(d), d if len(d) else np.zeros((1, o.n_rings, o.n_sectors), np.float32), ctypes.byref(o), cap, q, w, r, s, dist, yaw)
    m = min(n, cap)
    return n, [(int(q[k]), int(w[k]), int(r[k]), int(s[k]), float(dist[k]), float(yaw[k])) for k in range(m)]


def test_host_binning_matches_oracle(emul):
    """Every point of the two-lap fixture: the header's cell and value against numpy's, the descriptors and ring keys bit for
    bit; and every point lies at least 1e-9 (relative) from every ring, sector and range boundary."""
    desc, keys = pc.descriptors()
    worst = np.inf
    for f, cloud in enumerate(pc.clouds()):
        b = po.bins(cloud, **pc.PLACE)
        cell, h, D, key = host_descriptor(emul, cloud, **pc.PLACE)
        want = np.where(b["keep"], b["ring"] * pc.PLACE["n_sectors"] + b["sector"], -1)
        assert np.array_equal(cell, want) and np.array_equal(h[b["keep"]], b["h"][b["keep"]])
        assert D.tobytes() == desc[f].tobytes() and key.tobytes() == keys[f].tobytes()
        assert b["keep"].sum() > 2000 and (~b["keep"]).any()
        worst = min(worst, float(b["margin"].min()))
    print(f"smallest relative distance of a point to a bin or range boundary: {worst:.2e}")
    assert worst >= 1e-9
    # what no cloud of the fixture has: points that are not finite, below the floor, on the axis, at the outer range
    odd = np.float32([[np.nan, 1, 0], [1, np.inf, 0], [1, 1, np.nan], [1, 1, np.inf], [1, 1, -3.0], [0, 0, 1], [-1, 0, 0], [-1, -1e-30, 0],
                      [8, 0, 0], [7.9999995, 0, 1], [0.3, 0, 0], [0, -0.3, 0.25]])
    b = po.bins(odd, **pc.PLACE)
    cell, h, D, key = host_descriptor(emul, odd, **pc.PLACE)
    assert list(b["keep"]) == [False] * 6 + [True, True, False, True, True, True]
    assert np.array_equal(cell, np.where(b["keep"], b["ring"] * 60 + b["sector"], -1))
    assert D.tobytes() == po.descriptor(odd, **pc.PLACE)[0].tobytes()
    assert cell[6] == 2 * 60 + 59 and cell[7] == 2 * 60 + 0 and cell[9] // 60 == 19            # atan2 = pi: the last sector; -pi: the first


def test_rotation_sign_and_key_invariance():
    """A cloud turned by m sector angles about z: the query Rz(-m a) p against p has shift m (yaw = +m a: the query's body is
    the other body turned by +m a), and the ring key does not change."""
    rng = np.random.default_rng(4)
    ang = rng.uniform(-np.pi, np.pi, 4000)
    ang = np.floor(ang / pc.SECTOR) * pc.SECTOR + rng.uniform(0.2, 0.8, 4000) * pc.SECTOR      # away from the sector boundaries
    rad, z = rng.uniform(0.5, 7.5, 4000), rng.uniform(-2.0, 1.0, 4000)
    cloud = np.c_[rad * np.cos(ang), rad * np.sin(ang), z]
    D0, k0 = po.descriptor(cloud.astype(np.float32), **pc.PLACE)
    for m in (1, 7, 31, 59):
        turned = (cloud @ po.rz(-m * pc.SECTOR).T).astype(np.float32)
        D1, k1 = po.descriptor(turned, **pc.PLACE)
        d = po.shift_distances(D1, D0)
        assert int(np.argmin(d)) == m and d[m] < 1e-12 and k1.tobytes() == k0.tobytes()
        assert D1.tobytes() == np.roll(D0, -m, axis=1).tobytes()
    assert po.yaw_of(0, 60) == 0.0 and po.yaw_of(30, 60) == pytest.approx(po.PI) and po.yaw_of(31, 60) < 0 and po.yaw_of(59, 60) == pytest.approx(-pc.SECTOR)


def test_host_search_matches_oracle(emul):
    """The header's orders and selection, case by case, against numpy: the same lists, distances and yaws bit for bit."""
    for k, (name, desc, o, cap) in enumerate(pc.search_cases()):
        want, margin = pc.search_oracle(k)
        n, got = host_search(emul, desc, capacity=cap, **o)
        print(f"{name}: {n} candidates, decision margin {margin:.2e}")
        assert n == len(want) and got == want[:len(got)], name
        assert len(got) == (len(want) if cap is None else min(cap, len(want)))
        assert margin >= 1e-9, name
    want, margin = pc.candidates()
    n, got = host_search(emul, pc.descriptors()[0], **pc.PLACE)
    assert n == len(want) == 24 and got == want
    assert host_search(emul, np.zeros((0, 20, 60), np.float32), **pc.PLACE) == (0, [])


def test_synthetic_sets_cover_every_clause():
    cases = {c[0]: (k, c) for k, c in enumerate(pc.search_cases())}
    desc, roll = pc.syn(20, 60)
    assert len(desc) == 130 > 2 * 64 and not desc[77].any() and (desc >= 0).all() and desc.max() < 4.0
    assert any(not d.any(0).all() for d in desc[:40])                                               # empty columns
    assert desc[80].tobytes() == desc[0].tobytes() and desc[40].tobytes() != np.roll(desc[0], roll[40], 1).tobytes()
    full, _ = pc.search_oracle(cases["defaults-like"][0])
    cut, _ = pc.search_oracle(cases["cut to 1"][0])
    # exact ties in distance, resolved by w: a duplicate pair at distance 0 to the bit, the lower submap kept by the cut
    per_query = {}
    for c in full:
        per_query.setdefault(c[0], []).append(c)
    tied = [v for v in per_query.values() if len(v) == 2 and v[0][4] == v[1][4]]
    assert tied and all((v[0][0], v[0][1]) in {(c[0], c[1]) for c in cut} for v in tied)
    assert len(cut) < len(full)                                                 # more eligible submaps than max_per_frame
    # rolled copies: shift = the difference of the rolls
    ns = 60
    rolled = [c for c in full if roll[c[0]] != roll[c[2]]]
    assert rolled and all(c[3] == (roll[c[2]] - roll[c[0]]) % ns for c in rolled if c[0] % 40 == c[2] % 40)
    # the all-zero descriptor: distance 1 to everything, a candidate only at max_distance = 1
    assert not any(77 in (c[0], c[2]) for c in full)
    one, _ = pc.search_oracle(cases["max_distance 1"][0])
    assert [c[4] for c in one if c[0] == 77] and all(c[4] == 1.0 and c[3] == 0 for c in one if c[0] == 77)
    # more eligible frames than K: with every frame its own submap and K = 32 a query keeps 32 of 130
    k32, _ = pc.search_oracle(cases["K = 32, one submap per frame"][0])
    assert max(sum(1 for c in k32 if c[0] == q) for q in {c[0] for c in k32}) > 20
    assert {c[0] % 2 for c in pc.search_oracle(cases["query_stride 2"][0])[0]} == {0}
    assert cases["capacity"][1][3] < len(pc.search_oracle(cases["capacity"][0])[0])
    assert {(c[1][2]["n_rings"], c[1][2]["n_sectors"]) for c in cases.values()} >= {(20, 60), (7, 13), (10, 90), (32, 128)}


def test_two_lap_fixture_meets_its_conditions():
    """Lap B coincides with lap A in position; every lap-B query's one candidate is its own position's submap of lap A with
    ref = k and the planted shift; every decision has a margin >= 1e-9; the pose-based rule finds nothing at the drifted
    poses; and the oracle registers and accepts the lap-B candidates from T_init."""
    P = pc.truth()
    assert np.array_equal(P[:12, 9:], pc.lap_b_positions()) and np.array_equal(P[12:, 9:], pc.lap_b_positions())
    cand, margin = pc.candidates()
    print(f"decision margin {margin:.2e}")
    assert margin >= 1e-9
    lap_b = [c for c in cand if c[0] >= 12]
    assert [c[:4] for c in lap_b] == [(12 + k, k // 3, k, pc.planted(k)) for k in range(12)]
    assert all(c[4] <= 0.2 for c in lap_b)
    assert pc.pose_candidates(pc.drifted()) == [] and len(pc.pose_candidates(pc.truth())) == 24
    x = pc.drifted()
    assert min(np.linalg.norm(x[12 + k, 9:] - x[f, 9:]) for k in range(12) for f in range(12)) > pc.POSE_RADIUS
    accepted = 0
    for q, w, ref, s, d, yaw in lap_b:
        start, reg, (ok, why) = pc.oracle_register(q, w, ref, s)
        assert min(t["margin"] for t in reg["trace"]) >= 1e-9
        accepted += ok
        print(f"query {q} -> submap {w}, ref {ref}, shift {s}: {ro.CONVERGED == reg['status']}, inliers {reg['inliers']}, rmse {reg['rmse']:.4f}, {ok} {why}")
    assert accepted >= 8


def test_place_struct_sizes_match_the_header():
    L = importlib.import_module("global-lvba_amd._lib")
    # the mirrors against the header: tests/test_abi.py, every struct at once; here the check program's own copy of the options
    assert ctypes.sizeof(L.PlaceOpts) == 64 == ctypes.sizeof(EmulOpts) and ctypes.sizeof(L.PlaceCandidate) == 32
    assert all(s in L.SYMBOLS for s in ("lvba_place_default_opts", "lvba_place_descriptors", "lvba_place_search", "lvba_place_candidates"))
