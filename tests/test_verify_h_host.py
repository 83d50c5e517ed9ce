"""CPU tests of the homography model of the two-view verification and of the E-or-H choice (include/lvba_hip.h "The homography
model and the E-or-H choice"): csrc/verify_device.h on the host (tests/verify_h_check.cpp) against the numpy
oracle (tests/verify_h_oracle.py) to the bit, the refit under the measured tolerance, the margin condition of the fixtures
(tests/verify_h_cases.py), what the fixtures claim, the Python plumbing, and the same header under the host sanitizers in a
stand-alone program."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import match_oracle as mo
import verify_h_cases as hc
import verify_h_oracle as ho
import verify_oracle as vo
from host_build import build_check

# The largest difference between a refit of the host emulation (cyclic Jacobi) and the oracle's (LAPACK eigh) over all fixtures,
# entry by entry, both of unit norm and of the sign the rule fixes, measured on the CPU: 1.16e-13
# (test_refits_agree_within_the_measured_tolerance prints it; the eigen-gap of a homography's N is wider than that of the
# eight-point N, so d is smaller).  The tests allow ten times that, as the essential refits do.
REFIT_D = 1.2e-13
REFIT_TOL = 10 * REFIT_D
NEW_SYMBOLS = ("lvba_verify_pairs_model", "lvba_verify_hypotheses_homography", "lvba_verify_score_homography")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/verify_device.h compiled for the host, without contraction (tests/verify_h_check.cpp)"""
    lib = ctypes.CDLL(build_check("verify_h_check", tmp_path_factory.mktemp("emul_verify_h")))
    P = ctypes.c_void_p
    lib.emul_h_score.argtypes = [ctypes.c_int32, P, P, ctypes.c_double, P]
    lib.emul_h_score.restype = None
    lib.emul_h_hypotheses.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, ctypes.c_double, P, P, P]
    lib.emul_h_refit.argtypes = [ctypes.c_int32, P, ctypes.c_double, P, P]
    lib.emul_h_status.argtypes = [ctypes.c_int32] * 3
    lib.emul_h_choose.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_double]
    return lib


def tau2_of(case, **over):
    o = hc.options(case, **over)
    return mo.tau2(o["intr"], o["max_error_px"])


def host_hypotheses(emul, case):
    o = hc.options(case)
    P = np.ascontiguousarray(hc.case_points(case))
    H = o["hypotheses"]
    Hm, G, count = np.zeros((H, 9)), np.zeros((H, 9)), np.full(H, -1, np.int32)
    win = -1
    if len(P) >= ho.K:
        win = emul.emul_h_hypotheses(o["seed"], min(case["a"], case["b"]), max(case["a"], case["b"]), H, len(P), P.ctypes.data, tau2_of(case),
                                     Hm.ctypes.data, G.ctypes.data, count.ctypes.data)
    return Hm, G, count, win


def host_refit(emul, case, Hm):
    P = np.ascontiguousarray(hc.case_points(case))
    F = np.zeros(9)
    ok = emul.emul_h_refit(len(P), P.ctypes.data, tau2_of(case), np.ascontiguousarray(Hm, np.float64).ctypes.data, F.ctypes.data)
    return F if ok else None


def test_device_header_on_the_host_equals_the_oracle(emul):
    """Every hypothesis's H, G and count, the winner and the masks of every fixture the GPU tests use, bit for bit."""
    seen = 0
    for case in hc.all_cases():
        Hm, count, idx, _ = hc.oracle_hypotheses(case)
        gH, gG, gcount, win = host_hypotheses(emul, case)
        np.testing.assert_array_equal(gH, Hm, err_msg=case["name"])
        np.testing.assert_array_equal(gG, ho.inverse(Hm)[0], err_msg=case["name"])
        np.testing.assert_array_equal(gcount, count, err_msg=case["name"])
        assert win == vo.pick(count)[0], case["name"]
        seen += int((count >= 0).sum())
        if win >= 0:
            P = np.ascontiguousarray(hc.case_points(case))
            mask = np.zeros(len(P), np.uint8)
            emul.emul_h_score(len(P), P.ctypes.data, np.ascontiguousarray(Hm[win]).ctypes.data, tau2_of(case), mask.ctypes.data)
            np.testing.assert_array_equal(mask.astype(bool), ho.score(Hm[win], P, tau2_of(case)))
            assert mask.sum() == count[win]
    assert seen > 10000
    # a matrix without an inverse direction takes nothing in
    case = hc.cases()["planar_claims"][0]
    P = np.ascontiguousarray(hc.case_points(case))
    for M in (np.zeros(9), np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1]), np.full(9, np.nan)):
        mask = np.ones(len(P), np.uint8)
        emul.emul_h_score(len(P), P.ctypes.data, M.ctypes.data, tau2_of(case), mask.ctypes.data)
        assert not mask.any() and not ho.score(M, P, tau2_of(case)).any()
    for m, mi, c, want in ((3, 0, -1, vo.TOO_FEW_MATCHES), (14, 15, 14, vo.TOO_FEW_MATCHES), (4, 0, -1, vo.NO_MODEL), (40, 15, 14, vo.TOO_FEW_INLIERS),
                           (40, 15, 15, vo.OK), (4, 0, 0, vo.OK)):
        assert emul.emul_h_status(m, mi, c) == want
    # the choice, on both sides of its bound and where a run is not OK
    for sE in range(4):
        for sH in range(4):
            for nE, nH in ((10, 8), (10, 7), (15, 12), (15, 13), (0, 0), (100, 80), (100, 79), (36, 60)):
                for ratio in (0.8, 1.0, 0.5):
                    want = ho.choose(dict(status=sE, n_inliers=nE), dict(status=sH, n_inliers=nH), ratio)
                    assert emul.emul_h_choose(sE, nE, sH, nH, ratio) == want, (sE, nE, sH, nH, ratio)
    for nE in range(5, 400, 5):          # the bound itself, as fp64 rounds the product: at, and one below, 4/5 of n_E
        for nH in (4 * nE // 5, 4 * nE // 5 - 1):
            assert emul.emul_h_choose(0, nE, 0, nH, 0.8) == (ho.HOMOGRAPHY if float(nH) >= 0.8 * float(nE) else ho.ESSENTIAL)
    assert ho.choose(dict(status=0, n_inliers=10), dict(status=0, n_inliers=8)) == ho.HOMOGRAPHY
    assert ho.choose(dict(status=0, n_inliers=10), dict(status=0, n_inliers=7)) == ho.ESSENTIAL


def test_hypotheses_satisfy_their_own_samples():
    """a homography carries its four sample points of lo onto those of hi, in front of the camera, and back; unit norm"""
    for case in hc.cases()["planar_claims"][:2]:
        Hm, count, idx, _ = hc.oracle_hypotheses(case)
        P = hc.case_points(case)
        ok = count >= 0
        assert ok.mean() > 0.9
        np.testing.assert_allclose(np.linalg.norm(Hm[ok], axis=1), 1.0, atol=1e-14)
        S = P[idx[ok]]
        xl = np.concatenate([S[..., :2], np.ones(S.shape[:2] + (1,))], -1)
        p = np.einsum("hij,hkj->hki", Hm[ok].reshape(-1, 3, 3), xl)
        assert (p[:, 0, 2] > 0).all()                                   # the sign rule, at the first sample point
        well = np.abs(p[..., 2]).min(axis=1) > 1e-3                     # a sample with a wrong match may send a point far away
        assert well.mean() > 0.5
        assert np.abs(p[well][..., :2] / p[well][..., 2:] - S[well][..., 2:]).max() < 1e-7
        G, gok = ho.inverse(Hm[ok])
        assert gok.all()
        I = np.einsum("hij,hjk->hik", G.reshape(-1, 3, 3), Hm[ok].reshape(-1, 3, 3))
        assert (I[:, 0, 0] > 0).all()                                   # G is a positive multiple of the inverse
        assert np.abs(I - I[:, :1, :1] * np.eye(3)).max() < 1e-14       # G H = |det H| I up to the rounding of entries below 2


def test_fixture_margins():
    """No decision of a valid hypothesis of any fixture the GPU tests use -- the two distance tests, p2 > 0, q2 > 0, the sign at
    the first sample point, det H != 0 -- is within 1e-9 relative of its bound: zero exclusions."""
    worst = np.inf
    for case in hc.all_cases():
        worst = min(worst, hc.oracle_hypotheses(case)[3])
    print("smallest relative margin of any (fixture, hypothesis, match):", worst)
    assert worst >= hc.MIN_MARGIN, worst


def test_fixture_claims():
    c = hc.cases()
    # the homography on the plane at 30 %, 60 %, 70 % and 80 % outliers: exactly the planted set
    for case in c["planar_claims"]:
        r = hc.oracle_pair(case)
        assert r["status"] == vo.OK, case["name"]
        np.testing.assert_array_equal(r["mask"], case["planted"], err_msg=case["name"])
        rE = hc.oracle_pair_E(case)
        print(case["name"], "planted", int(case["planted"].sum()), "homography", r["n_inliers"], "eight-point", rE["n_inliers"], "wrong ones it keeps",
              int((rE["mask"] & ~case["planted"]).sum()), "H / E", r["n_inliers"] / max(rE["n_inliers"], 1))
    # AUTO with method 0: HOMOGRAPHY on the plane, ESSENTIAL in general position, exactly the planted set on all of them
    for case in c["planar_claims"] + c["general_claims"]:
        r = hc.oracle_auto(case)
        assert r["kind"] == (ho.HOMOGRAPHY if case["name"].startswith("planar") else ho.ESSENTIAL), case["name"]
        assert r["status"] == vo.OK
        np.testing.assert_array_equal(r["mask"], case["planted"], err_msg=case["name"])
        ratio = r["n_inliers_H"] / r["n_inliers_E"]
        print(case["name"], "n_H / n_E =", ratio)
        assert ratio >= 0.85 if r["kind"] == ho.HOMOGRAPHY else ratio <= 0.3         # either side of planar_ratio = 0.8, with room
    assert c["general_claims"][1]["a"] > c["general_claims"][1]["b"]                 # one pair given as (hi, lo)
    # a NaN point is never an inlier, and a sample that holds one is invalid
    case = c["general_claims"][1]
    P = hc.case_points(case)
    nan = np.isnan(P).any(axis=1)
    Hm, count, idx, _ = hc.oracle_hypotheses(case)
    assert nan.sum() == 3 and (count[nan[idx].any(axis=1)] == -1).all() and nan[idx].any(axis=1).sum() > 0
    assert not ho.score(Hm[vo.pick(count)[0]], P, tau2_of(case))[nan].any()
    # one match repeated, and three sample points on a line whose matches are on a line: every hypothesis loses a pivot
    for case in c["special"] + c["collinear"]:
        Hm, count, _, _ = hc.oracle_hypotheses(case)
        assert (count == -1).all() and not Hm.any(), case["name"]
        r = hc.oracle_pair(case, min_inliers=0)
        assert r["status"] == vo.NO_MODEL and r["best_h"] == -1 and not r["E"].any() and not r["mask"].any()
    # (hi, lo) is (lo, hi) with the columns exchanged
    r0, r1 = (hc.oracle_pair(k) for k in c["flipped"])
    np.testing.assert_array_equal(r0["E"], r1["E"]); np.testing.assert_array_equal(r0["mask"], r1["mask"])
    assert r0["status"] == vo.OK
    # the statuses of the size ladder
    for case in c["sizes"]:
        assert (hc.oracle_pair(case)["status"] == vo.TOO_FEW_MATCHES) == (len(case["matches"]) < 15), case["name"]
        assert (hc.oracle_pair(case, min_inliers=0)["status"] == vo.TOO_FEW_MATCHES) == (len(case["matches"]) < ho.K), case["name"]
    # the mixed batch decides both ways, and every pair it calls OK under AUTO keeps no wrong match
    kinds = [hc.oracle_auto(k) for k in c["mixed"]]
    big = [(k, r) for k, r in zip(c["mixed"], kinds) if len(k["matches"]) >= 60]
    assert all(r["kind"] == (ho.HOMOGRAPHY if k["planar"] else ho.ESSENTIAL) for k, r in big) and len(big) > 20
    assert {r["kind"] for r in kinds} == {ho.ESSENTIAL, ho.HOMOGRAPHY}


def test_refits_agree_within_the_measured_tolerance(emul):
    """The host emulation's refit (cyclic Jacobi) against the oracle's (LAPACK eigh) from the same H over the same inliers."""
    d, n, worst = 0.0, 0, None
    for case in hc.all_cases():
        if len(case["matches"]) < 15:
            continue
        Hm, count, _, _ = hc.oracle_hypotheses(case)
        h, c = vo.pick(count)
        if h < 0:
            continue
        P = hc.case_points(case)
        tau2 = tau2_of(case)
        cur = Hm[h]
        for rnd in range(2):
            want, got = ho.refit(cur, P, tau2), host_refit(emul, case, cur)
            assert (want is None) == (got is None), case["name"]
            if want is None:
                break
            assert abs(np.linalg.norm(got) - 1.0) < 1e-14 and got @ cur > 0
            if c >= 30:             # a refit over a handful of inliers has no eigen-gap to speak of
                e = float(np.abs(got - want).max())
                if e > d:
                    d, worst = e, (case["name"], rnd)
                n += 1
            cn = int(ho.score(got, P, tau2).sum())
            if cn <= c:             # the rule stops here too
                break
            cur, c = got, cn
    print("largest refit difference d over", n, "refits:", d, "in", worst)
    assert n > 30 and d <= REFIT_D
    # where the winner misses planted matches the refit finds them: planar-80% goes from 57 to the 60 planted
    case = hc.cases()["planar_claims"][3]
    r0, r = hc.oracle_pair(case, refine_rounds=0), hc.oracle_pair(case)
    print("planar-80%: inliers before the refit", r0["n_inliers"], "after", r["n_inliers"])
    assert r0["n_inliers"] <= r["n_inliers"] == int(case["planted"].sum())


class RecordingLib:
    """stands in for the library: every entry point returns 0 and its name is recorded"""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        if not name.startswith("lvba_"):
            raise AttributeError(name)
        self.names.append(name)
        return lambda *a: 0


def test_the_default_model_is_the_old_entry_point(monkeypatch):
    """Verifier.pairs / pairs_csr / verify_pairs and run_full_pipeline(verify_matches=...) without `model`, and with
    model="essential", call lvba_verify_pairs and look none of the new symbols up; "homography" and "auto" look
    lvba_verify_pairs_model up."""
    L = importlib.import_module("global-lvba_amd._lib")
    VF = importlib.import_module("global-lvba_amd.verify")
    pl = importlib.import_module("global-lvba_amd.pipeline")
    lib = RecordingLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    kps = [np.zeros((5, 2), np.float32)] * 2
    mm = [np.array([[0, 1], [2, 3]], np.int32)]
    for kw in ({}, dict(model="essential"), dict(model=0, planar_ratio=0.5)):
        lib.names.clear()
        inl, rep = VF.verify_pairs(kps, [(0, 1)], mm, np.ones(8), **kw)
        assert "lvba_verify_pairs" in lib.names and not set(lib.names) & set(NEW_SYMBOLS), (kw, lib.names)
        assert "kind" not in rep and "n_inliers_E" not in rep and "model" not in VF.summary([(0, 1)], rep)["pairs"][0]
        with VF.Verifier(kps, np.ones(8)) as v:
            v.hypotheses(0, 1, mm[0], hypotheses=4, **({"model": kw["model"]} if "model" in kw else {}))
            v.score(0, 1, mm[0], np.eye(3))
        assert not set(lib.names) & set(NEW_SYMBOLS), lib.names
    for model in ("homography", "auto", 1, 2):
        lib.names.clear()
        inl, rep = VF.verify_pairs(kps, [(0, 1)], mm, np.ones(8), model=model)
        assert "lvba_verify_pairs_model" in lib.names and "lvba_verify_pairs" not in lib.names
        s = VF.summary([(0, 1)], rep)
        assert {"kind", "n_inliers_E", "n_inliers_H"} <= set(rep) and s["pairs"][0]["model"] == "essential" and "n_pairs_planar" in s
    with pytest.raises(ValueError):
        VF.verify_pairs(kps, [(0, 1)], mm, np.ones(8), model="plane")
    with VF.Verifier(kps, np.ones(8)) as v:
        lib.names.clear()
        v.hypotheses(0, 1, mm[0], model="homography", hypotheses=4)
        v.score_homography(0, 1, mm[0], np.eye(3))
        assert lib.names == ["lvba_verify_default_opts", "lvba_verify_hypotheses_homography", "lvba_verify_score_homography"]
        with pytest.raises(ValueError):
            v.hypotheses(0, 1, mm[0], model="auto")

    class FakeScans:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *e):
            pass

    monkeypatch.setattr(pl, "Scans", FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: {})
    args = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
            np.ones(8), 640, 512, kps, [(0, 1)], mm)
    for vm, new in ((dict(method=0), False), (dict(method=0, model="essential"), False), (dict(method=0, model="auto"), True)):
        lib.names.clear()
        out = pl.run_full_pipeline(*args, enable_lidar_ba=False, verify_matches=vm)
        assert bool(set(lib.names) & set(NEW_SYMBOLS)) == new, (vm, lib.names)
        rec = out["match_verification"]["pairs"][0]
        assert ("model" in rec) == new and ("n_pairs_planar" in out["match_verification"]) == new


def test_run_dataset_hands_the_model_on(tmp_path, monkeypatch):
    """run_dataset(verify=dict(model=...)) passes the keywords to run_full_pipeline untouched and writes the report's new fields
    to match_verification.json."""
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
    report = dict(pairs=[dict(pair=[0, 1], status="too_few_matches", n_matches=2, n_inliers=0, model="essential", n_inliers_E=0, n_inliers_H=0)],
                  n_pairs=1, n_pairs_ok=0, n_matches=2, n_inliers=0, n_pairs_planar=0)
    monkeypatch.setattr(pl, "run_full_pipeline",
                        lambda *a, **k: calls.append(k) or dict({"match_verification": report} if k.get("verify_matches") else {},
                                                                   poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1))))
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir), verify=dict(model="auto", planar_ratio=0.7, method=0))
    assert calls[0]["verify_matches"] == dict(model="auto", planar_ratio=0.7, method=0)
    assert json.load(open(out_dir / "match_verification.json")) == report


def test_the_header_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/verify_h_check.cpp as a stand-alone program (its own main: hypotheses, refit, score and choice on a synthetic plane
    with wrong matches and a NaN point) built with -fsanitize=address,undefined: it runs clean and finds the planted set."""
    exe = build_check("verify_h_check", tmp_path, shared=False,
                      flags=("-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas"),
                      extra=("-DVERIFY_H_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))     # the leak checker needs ptrace, which a sandbox may deny
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "inliers 30 wrong 0" in r.stdout and "runtime error" not in r.stderr
