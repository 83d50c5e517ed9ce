"""CPU tests of the descriptor matcher's rule and fixtures (include/lvba_hip.h "descriptor matching of image pairs"):
the numpy oracle against the definition as plain loops, the signed-byte identity of the kernel, the margin condition of the
fixtures, the repeated-texture claim of the guided gate, the descriptor loader, and run_dataset's default path."""
import ctypes
import importlib
import sqlite3
import sys

import numpy as np
import pytest

import match_cases as mc
import match_oracle as mo
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/match_device.h compiled for the host, without contraction, walked as the kernel walks it (tests/match_check.cpp)"""
    lib = ctypes.CDLL(build_check("match_check", tmp_path_factory.mktemp("emul_match")))
    for f in (lib.emul_essential, lib.emul_undistort, lib.emul_scan):
        f.restype = None
    lib.emul_scan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emul_undistort.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emul_essential.argtypes = [ctypes.c_void_p] * 5
    lib.emul_accept.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double]
    return lib


def host_scan(emul, descs, a, b, geom=None, max_epipolar_px=4.0):
    A, B = descs[a], descs[b]
    best, s1, s2 = (np.zeros(max(len(A), 1), np.int32) for _ in range(3))
    E, xa, xb, t2 = np.zeros(9), np.zeros(2), np.zeros(2), 0.0
    if geom is not None:
        lo, hi = min(a, b), max(a, b)
        E = np.zeros(9)
        emul.emul_essential(*(np.ascontiguousarray(x).ctypes.data for x in (geom.R[lo], geom.t[lo], geom.R[hi], geom.t[hi])), E.ctypes.data)
        np.testing.assert_array_equal(E.reshape(3, 3), mo.essential(geom.R[lo], geom.t[lo], geom.R[hi], geom.t[hi]))
        xa, xb = np.ascontiguousarray(geom.xy[a]), np.ascontiguousarray(geom.xy[b])
        t2 = mo.tau2(geom.intr, max_epipolar_px)
    emul.emul_scan(len(A), len(B), A.ctypes.data, B.ctypes.data, int(geom is not None), int(a < b), E.ctypes.data, xa.ctypes.data,
                   xb.ctypes.data, t2, best.ctypes.data, s1.ctypes.data, s2.ctypes.data)
    return best[:len(A)], s1[:len(A)], s2[:len(A)]


def test_device_header_on_the_host_equals_the_oracle(emul):
    """The kernel's arithmetic without the GPU: signed bytes and the bias as the accumulator's start, per-lane running top two, the
    butterfly merge, the gate's expressions without contraction, the essential matrix and the undistortion bit for bit."""
    u = mc.unguided()
    for a, b in ((2, 4), (4, 2), (7, 6), (1, 6), (6, 1), (6, 0), (6, u["DUP_B"]), (u["DUP_B"], 6), (u["DUP_A"], 6), (u["EXT"], 6),
                 (6, u["EXT"]), (u["EXT"], u["DUP_B"])):
        for got, want in zip(host_scan(emul, u["descs"], a, b), mo.scan(u["descs"], a, b)):
            np.testing.assert_array_equal(got, want, err_msg=f"pair ({a}, {b})")
    g = mc.guided()
    for second in (False, True):
        geo = mc.guided_geometry(second)
        for k, uv in enumerate(g["keypoints"]):
            xy = np.zeros((len(uv), 2))
            emul.emul_undistort(len(uv), np.ascontiguousarray(uv, np.float32).ctypes.data, geo.intr.ctypes.data, xy.ctypes.data)
            np.testing.assert_array_equal(xy, geo.xy[k])
        for a, b in ((0, 1), (1, 0), (3, 1), (0, 4), (4, 1)):
            for px in (4.0, 1.5):
                for got, want in zip(host_scan(emul, g["descs"], a, b, geo, px), mo.scan(g["descs"], a, b, geo, guided=1, max_epipolar_px=px)):
                    np.testing.assert_array_equal(got, want, err_msg=f"pair ({a}, {b}) at {px} px")
    best, s1, s2 = mo.scan(u["descs"], 8, 9)
    want = (best >= 0) & (mo.distance(s1) < 0.7) & (mo.distance(s1) < 0.8 * mo.distance(s2))
    got = [emul.emul_accept(int(b), int(x), int(y), 0.7, 0.8) for b, x, y in zip(best, s1, s2)]
    np.testing.assert_array_equal(np.array(got, bool), want)


def test_oracle_equals_the_definition_as_loops():
    u = mc.unguided()
    d = u["descs"]
    for a, b in ((2, 4), (4, 2), (1, 6), (6, 1), (0, 6), (6, 0), (1, 0), (6, u["DUP_B"]), (u["DUP_A"], 6), (u["EXT"], 6), (6, u["EXT"])):
        for got, want in zip(mo.scan(d, a, b), mo.brute_scan(d[a], d[b])):
            np.testing.assert_array_equal(got, want)
    g, geo = mc.guided(), mc.guided_geometry()
    A, B = g["descs"][0][:20], g["descs"][1][:25]
    mask = geo.mask(0, 1, 4.0)[:20, :25]
    for got, want in zip(mo.top_two(mo.scores(A, B), mask), mo.brute_scan(A, B, mask)):
        np.testing.assert_array_equal(got, want)


def test_top_two_edge_rules():
    u = mc.unguided()
    d = u["descs"]
    best, s1, s2 = mo.scan(d, 6, 1)                         # one column: s2 = 0, d2 = pi / 2
    assert (best == 0).all() and (s2 == 0).all() and mo.distance(0) == np.pi / 2
    best, s1, s2 = mo.scan(d, 6, 0)                         # no column at all
    assert (best == -1).all() and (s1 == 0).all() and (s2 == 0).all()
    best, s1, s2 = mo.scan(d, 6, u["DUP_B"])                # duplicates among the columns: the lowest, s2 = s1, ratio rejects
    assert best[7] == 7 and s1[7] == s2[7]
    m, _ = mo.match_pair(d, 6, u["DUP_B"])
    assert 7 not in m[:, 0] and len(m) > 40
    m, _ = mo.match_pair(d, u["DUP_A"], 6, max_ratio=1.0, max_distance=1.5)   # duplicates among the rows: mutual keeps the lower
    assert 3 in m[:, 0] and 50 not in m[:, 0]
    m1, _ = mo.match_pair(d, u["DUP_A"], 6, max_ratio=1.0, max_distance=1.5, mutual=0)
    assert 3 in m1[:, 0] and 50 in m1[:, 0]
    best, s1, s2 = mo.scan(d, u["EXT"], 6)                  # all 0: every score 0, the lowest column; all 255: clamped to d = 0
    assert best[5] == 0 and s1[5] == 0 and s2[5] == 0
    assert s1[6] > 262144 and mo.distance(s1[6]) == 0.0 and mo.distance(s2[6]) == 0.0
    m, _ = mo.match_pair(d, u["EXT"], 6)
    assert not {5, 6} & set(m[:, 0].tolist())


def test_bias_identity():
    """sum a b = sum a'b' + 128 (sum a' + sum b') + 128^3 with a' = a - 128 a signed byte, |sum a'b'| <= 2^21: exact in int32"""
    rng = np.random.default_rng(3)
    A = np.vstack([mc.sift_like(rng, 50), np.zeros((1, 128), np.uint8), np.full((1, 128), 255, np.uint8),
                   rng.integers(0, 256, (20, 128)).astype(np.uint8)])
    B = A[::-1].copy()
    np.testing.assert_array_equal(mo.scores(A, B), mo.scores_biased(A, B))
    Ab = A.astype(np.int64) - 128
    assert np.abs(Ab @ Ab.T).max() <= 2 ** 21 and Ab.min() >= -128 and Ab.max() <= 127
    np.testing.assert_array_equal((A ^ 0x80).view(np.int8), Ab)          # the top bit flipped IS a - 128
    assert mo.scores(A, B).max() < 2 ** 23


def test_fixture_margins_and_clause_coverage():
    u = mc.unguided()
    assert mc.check_margins(u["descs"], u["pairs"], mc.OPTION_SETS) >= mc.MIN_MARGIN
    nd, nr, nm = mc.rejections(u["descs"], u["pairs"])
    assert nd > 0 and nr > 0 and nm > 0                                   # each of the three clauses rejects something
    nd, nr, nm = mc.rejections(u["descs"], u["pairs"], **mc.OPTION_SETS[2])
    assert nr > 100 and nm > 100
    g, geo = mc.guided(), mc.guided_geometry()
    assert mc.check_margins(g["descs"], g["pairs"], mc.GUIDED_OPTION_SETS, geo) >= mc.MIN_MARGIN
    assert mc.check_margins(g["descs"], g["pairs"], mc.GUIDED_OPTION_SETS[:1], mc.guided_geometry(second=True)) >= mc.MIN_MARGIN
    for a, b in ((8, 9), (2, 4), (7, 8)):                                 # the planted correspondences are what is found
        m, _ = mo.match_pair(u["descs"], a, b)
        pa, pb = u["planted"][a], u["planted"][b]
        assert len(m) and all(pa[r] >= 0 and pa[r] == pb[c] for r, c in m)


def test_guided_gate_recovers_repeated_texture():
    """Every repeated texture sits at 4 different 3-D points: the unguided ratio test finds none of them (best and second best
    are copies of one another); under the gate the copies lie off the epipolar line and the planted match comes back."""
    g, geo = mc.guided(), mc.guided_geometry()
    for a, b in ((0, 1), (1, 0), (0, 2), (3, 1), (2, 3)):
        rep, uniq = mc.planted_matches(g, a, b, True), mc.planted_matches(g, a, b, False)
        mu = set(map(tuple, mo.match_pair(g["descs"], a, b)[0].tolist()))
        mg = set(map(tuple, mo.match_pair(g["descs"], a, b, geo, guided=1)[0].tolist()))
        assert len(rep) >= 40 and not mu & rep
        assert len(mg & rep) >= 0.8 * len(rep) and not mg - rep - uniq      # most come back, and nothing wrong with them
        assert len(mg & uniq) >= len(mu & uniq) - 1                         # (the keypoint that fails to undistort)
    # the same decision from both sides: (b, a) is the transposed mask
    np.testing.assert_array_equal(geo.mask(0, 1, 4.0), geo.mask(1, 0, 4.0).T)
    # identical centres: no epipolar geometry, every candidate passes -> the unguided result
    assert not mo.essential(g["Rcw"][0], g["tcw"][0], g["Rcw"][4], g["tcw"][4]).any()
    np.testing.assert_array_equal(mo.match_pair(g["descs"], 0, 4, geo, guided=1)[0], mo.match_pair(g["descs"], 0, 4)[0])
    # a keypoint whose undistortion fails matches nothing, also in the pair without geometry
    bad = int(np.flatnonzero(np.isnan(g["keypoints"][1][:, 0]))[0])
    assert not geo.mask(1, 0, 4.0)[bad].any() and not geo.mask(4, 1, 4.0)[:, bad].any()
    assert bad in mo.match_pair(g["descs"], 1, 0)[0][:, 0]


def test_load_colmap_descriptors(tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    p = str(tmp_path / "db.db")
    con = sqlite3.connect(p)
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE descriptors (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    rng = np.random.default_rng(1)
    d7, d3 = mc.sift_like(rng, 9), mc.sift_like(rng, 4)
    for iid, name in ((7, "a.png"), (3, "b.png"), (9, "c.png"), (5, "d.png"), (6, "e.png")):
        con.execute("INSERT INTO images VALUES (?, ?)", (iid, name))
    con.execute("INSERT INTO descriptors VALUES (?, ?, ?, ?)", (7, 9, 128, d7.tobytes()))
    con.execute("INSERT INTO descriptors VALUES (?, ?, ?, ?)", (3, 4, 128, d3.tobytes()))
    con.execute("INSERT INTO descriptors VALUES (?, ?, ?, ?)", (9, 4, 128, d3.tobytes()[:-1]))       # a short blob
    con.execute("INSERT INTO descriptors VALUES (?, ?, ?, ?)", (5, 8, 64, d3.tobytes()))             # not 128 columns
    con.execute("INSERT INTO descriptors VALUES (?, ?, ?, ?)", (6, 2, 128, None))                    # no blob
    con.commit(); con.close()
    out = ds.load_colmap_descriptors(p, ["b.png", "a.png", "c.png", "d.png", "e.png", "missing.png"])
    np.testing.assert_array_equal(out[0], d3); np.testing.assert_array_equal(out[1], d7)
    assert all(o.shape == (0, 128) and o.dtype == np.uint8 for o in out[2:]) and out[0].dtype == np.uint8
    q = str(tmp_path / "nodesc.db")                                                                  # a database without the table
    con = sqlite3.connect(q)
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("INSERT INTO images VALUES (1, 'a.png')")
    con.commit(); con.close()
    assert ds.load_colmap_descriptors(q, ["a.png"])[0].shape == (0, 128)


def test_run_dataset_db_is_the_untouched_path(tmp_path, monkeypatch):
    """matching="db" (the default) hands run_full_pipeline exactly what the call without the argument hands it, and neither
    imports the match module nor loads the descriptors."""
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
    calls = []
    monkeypatch.setattr(pl, "run_full_pipeline", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(ds, "load_colmap_descriptors", lambda *a, **k: pytest.fail("the default path reads no descriptors"))
    sys.modules.pop("global-lvba_amd.match", None)
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    pl.run_dataset(*args)
    pl.run_dataset(*args, matching="db")
    assert "global-lvba_amd.match" not in sys.modules
    (a0, k0), (a1, k1) = calls
    assert k0.keys() == k1.keys() and "match_fn" not in k0
    assert len(a0) == len(a1)
    for x, y in zip(a0, a1):
        assert repr(x) == repr(y)
    np.testing.assert_array_equal(a0[-1][0], [[0, 1], [2, 3]])
    with pytest.raises(ValueError):
        pl.run_dataset(*args, matching="sift")
