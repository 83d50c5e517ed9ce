"""GPU tests of the two-view verification (lvba_verify_*, verify.Verifier, pipeline.verify_image_pairs) against the numpy
restatement (tests/verify_oracle.py) on the shared fixtures (tests/verify_cases.py).  A hypothesis is formed from
+, -, *, / and sqrt in one order and the file is built without contraction: E, counts, winners and inlier lists are compared
exactly.  Only the refits, which go through eig3 and Jacobi, are held to the tolerance measured in test_verify_host.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import match_oracle as mo
import verify_cases as vc
import verify_oracle as vo
from test_verify_host import REFIT_TOL

pytestmark = pytest.mark.gpu
MARGIN = 1e-9


@pytest.fixture(scope="module")
def VF(pkg):
    return importlib.import_module("global-lvba_amd.verify")


@pytest.fixture(scope="module")
def gen(VF):
    sc = vc.general()["scene"]
    with VF.Verifier(sc["keypoints"], sc["intr"], Rcw=sc["Rcw"]) as v:
        yield v


@pytest.fixture(scope="module")
def plane(VF):
    sc = vc.planar()["scene"]
    with VF.Verifier(sc["keypoints"], sc["intr"], Rcw=sc["Rcw"]) as v:
        yield v


def check_hypotheses(v, sc, case):
    E, count, _, _ = vc.oracle_hypotheses(sc, case)
    gE, gcount = v.hypotheses(case["a"], case["b"], case["matches"], **case["opts"])
    np.testing.assert_array_equal(gE.reshape(-1, 9), E, err_msg=case["name"])
    np.testing.assert_array_equal(gcount, count, err_msg=case["name"])


def want_batch(sc, cases, **over):
    rs = [vc.oracle_pair(sc, c, **over) for c in cases]
    inl = [c["matches"][r["mask"]] for c, r in zip(cases, rs)]
    return rs, inl


def run_batch(v, cases, **over):
    o = dict(cases[0]["opts"], **over)
    return v.pairs([(c["a"], c["b"]) for c in cases], [c["matches"] for c in cases], **o)


def check_batch_exact(got, want, names):
    (ginl, rep), (rs, winl) = got, want
    np.testing.assert_array_equal(rep["status"], [r["status"] for r in rs])
    np.testing.assert_array_equal(rep["best_h"], [r["best_h"] for r in rs])
    np.testing.assert_array_equal(rep["n_inliers"], [r["n_inliers"] for r in rs])
    np.testing.assert_array_equal(rep["E"].reshape(-1, 9), np.array([r["E"] for r in rs]).reshape(-1, 9))
    for g, w, n in zip(ginl, winl, names):
        np.testing.assert_array_equal(g, w, err_msg=n)


def test_hypotheses_equal_the_oracle(gen, plane):
    """every hypothesis's E and count, bit for bit: the match-count ladder of both methods (either side of the sample size, of
    the wavefront and of the LDS chunk), H either side of the hypothesis block, NaN keypoints, one match repeated, the plane"""
    g, p = vc.general(), vc.planar()
    for case in g["sizes"][0] + g["sizes"][1] + g["h_edges"] + g["special"] + g["claims"][2:] + g["flipped"]:
        check_hypotheses(gen, g["scene"], case)
    for case in p["claims"]:
        check_hypotheses(plane, p["scene"], case)
    nanh = vc.oracle_hypotheses(g["scene"], g["claims"][2])
    assert (nanh[1] == -1).sum() > 0                           # the samples that hold a NaN point


def test_pairs_without_refinement_equal_the_oracle(gen, VF):
    g = vc.general()
    sc = g["scene"]
    for method in (0, 1):
        cases = g["mixed"][method]
        names = [c["name"] for c in cases]
        got = run_batch(gen, cases, refine_rounds=0)
        check_batch_exact(got, want_batch(sc, cases, refine_rounds=0), names)
        assert set(got[1]["status"].tolist()) >= {VF.OK, VF.TOO_FEW_MATCHES}
        np.testing.assert_array_equal(got[1]["n_matches"], [len(c["matches"]) for c in cases])
        # two identical calls, the pairs one at a time, and the batch reversed: the same bytes
        again = run_batch(gen, cases, refine_rounds=0)
        back = run_batch(gen, cases[::-1], refine_rounds=0)
        for k in ("E", "status", "n_inliers", "best_h"):
            assert got[1][k].tobytes() == again[1][k].tobytes() and got[1][k].tobytes() == back[1][k][::-1].tobytes(), k
        for a, b, c in zip(got[0], again[0], back[0][::-1]):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        for k in (0, 3, 7, 9, 17):
            one = run_batch(gen, cases[k:k + 1], refine_rounds=0)
            assert one[0][0].tobytes() == got[0][k].tobytes() and one[1]["E"][0].tobytes() == got[1]["E"][k].tobytes()
            assert one[1]["best_h"][0] == got[1]["best_h"][k]
    # no pair, one pair, the ladders with their own H, one match repeated
    inl, rep = gen.pairs(np.zeros((0, 2), np.int32), [])
    assert inl == [] and len(rep["status"]) == 0
    for case in g["sizes"][0] + g["sizes"][1] + g["h_edges"] + g["special"]:
        check_batch_exact(run_batch(gen, [case], refine_rounds=0), want_batch(sc, [case], refine_rounds=0), [case["name"]])
        check_batch_exact(run_batch(gen, [case], refine_rounds=0, min_inliers=0), want_batch(sc, [case], refine_rounds=0, min_inliers=0),
                          [case["name"]])
    for case in g["special"]:
        inl, rep = run_batch(gen, [case])
        assert rep["status"][0] == VF.NO_MODEL and rep["best_h"][0] == -1 and not rep["E"].any() and len(inl[0]) == 0
    # (hi, lo) is (lo, hi) with the columns swapped back
    (i0, r0), (i1, r1) = (run_batch(gen, [c]) for c in g["flipped"])
    assert r0["E"].tobytes() == r1["E"].tobytes() and r0["best_h"][0] == r1["best_h"][0]
    np.testing.assert_array_equal(i0[0], i1[0][:, ::-1])
    assert len(i0[0]) >= 15


def check_refined(v, sc, cases, planted_claim):
    base_inl, base = run_batch(v, cases, refine_rounds=0)
    inl, rep = run_batch(v, cases)
    excluded = total = 0
    for k, case in enumerate(cases):
        o = vc.options(sc, case)
        P = vc.case_points(sc, case)
        tau2 = mo.tau2(sc["intr"], o["max_error_px"])
        assert rep["n_inliers"][k] >= base["n_inliers"][k] and rep["best_h"][k] == base["best_h"][k]
        if rep["status"][k] != vo.OK:
            assert len(inl[k]) == 0
            continue
        want, rel = vo.score(rep["E"][k].reshape(9), P, tau2, with_margin=True)
        got = np.zeros(len(P), bool)
        i = 0
        for r in inl[k].tolist():                              # the inliers are a subsequence of the matches, in their order
            while case["matches"][i].tolist() != r:
                i += 1
            got[i] = True
            i += 1
        sure = rel > MARGIN
        np.testing.assert_array_equal(got[sure], want[sure], err_msg=case["name"])
        excluded += int((~sure).sum()); total += len(P)
        assert rep["n_inliers"][k] == got.sum()
        r = vc.oracle_pair(sc, case)
        if r["n_inliers"] >= 30 and case["name"] != "planar-60%-eight":
            d = vo.difference(rep["E"][k], r["E"])
            print(case["name"], "refined E against the oracle's:", d)
            assert d <= REFIT_TOL, (case["name"], d)
        if planted_claim and case["name"] != "planar-60%-eight":
            np.testing.assert_array_equal(got, case["planted"], err_msg=case["name"])
    assert excluded <= 0.01 * total, (excluded, total)


def test_pairs_with_refinement(gen, plane):
    g, p = vc.general(), vc.planar()
    for method in (0, 1):
        check_refined(gen, g["scene"], [c for c in g["claims"] if c["opts"]["method"] == method], True)
        check_refined(gen, g["scene"], g["mixed"][method], False)
    check_refined(plane, p["scene"], p["claims"][:1], True)
    # the rotation-aided refit where it is taken: from a single hypothesis the winner is poor and the refit counts more
    taken = 0
    for case in g["h_edges"]:
        if case["opts"]["method"] != 1:
            continue
        r0, r = vc.oracle_pair(g["scene"], case, refine_rounds=0), vc.oracle_pair(g["scene"], case)
        inl, rep = run_batch(gen, [case])
        assert rep["n_inliers"][0] == r["n_inliers"] and rep["best_h"][0] == r["best_h"] and rep["status"][0] == r["status"], case["name"]
        assert vo.difference(rep["E"][0], r["E"]) <= REFIT_TOL, case["name"]
        taken += int(r["n_inliers"] > r0["n_inliers"])
    assert taken >= 1
    check_refined(plane, p["scene"], p["claims"][1:], False)


def test_score_is_the_guided_matchers_gate(gen, plane):
    """under the true E of match_essential the mask is what the guided matcher's gate decides for the same E and tau"""
    for v, fx in ((gen, vc.general()), (plane, vc.planar())):
        sc = fx["scene"]
        geo = mo.Geometry(sc["keypoints"], sc["intr"], sc["Rcw"], sc["tcw"])
        for case in fx["claims"]:
            a, b, mm = case["a"], case["b"], case["matches"]
            for px in (4.0, 1.0):
                gate = geo.mask(a, b, px)                   # [n_a, n_b]
                got = v.score(a, b, mm, vc.true_E(sc, a, b), max_error_px=px)
                np.testing.assert_array_equal(got, gate[mm[:, 0], mm[:, 1]], err_msg=case["name"])
            np.testing.assert_array_equal(v.score(a, b, mm, vc.true_E(sc, a, b)), vo.score(vc.true_E(sc, a, b), vc.case_points(sc, case),
                                                                                          mo.tau2(sc["intr"], 4.0)))
            fin = ~np.isnan(vc.case_points(sc, case)).any(axis=1)
            assert v.score(a, b, mm, vc.true_E(sc, a, b))[case["planted"] & fin].all()


def test_error_paths(VF, gen, pkg):
    L = pkg._lib
    g = vc.general()
    sc, case = g["scene"], g["claims"][0]
    mm = case["matches"]
    with VF.Verifier(sc["keypoints"], sc["intr"]) as bare:             # no rotations
        with pytest.raises(L.LvbaError) as e:
            bare.pairs([(0, 1)], [mm], method=1)
        assert e.value.code == L.ERR_ARG and "Rcw" in str(e.value)
        inl, rep = bare.pairs([(0, 1)], [mm], refine_rounds=0)          # method 0 needs none, and is the same bytes
        assert rep["E"].tobytes() == gen.pairs([(0, 1)], [mm], refine_rounds=0)[1]["E"].tobytes()
    bad = mm.copy(); bad[7, 1] = len(sc["keypoints"][1])
    for pairs, ms, kw in (([(0, 0)], [mm], {}), ([(0, 4)], [mm], {}), ([(-1, 1)], [mm], {}), ([(0, 1)], [bad], {}),
                          ([(0, 1)], [-mm - 1], {}), ([(0, 1)], [mm], dict(hypotheses=0)), ([(0, 1)], [mm], dict(method=2)),
                          ([(0, 1)], [mm], dict(max_error_px=0.0))):
        with pytest.raises(L.LvbaError) as e:
            gen.pairs(pairs, ms, **kw)
        assert e.value.code == L.ERR_ARG
    with pytest.raises(L.LvbaError):
        gen.hypotheses(0, 1, bad)
    with pytest.raises(L.LvbaError):
        gen.score(1, 1, mm, np.eye(3))
    with pytest.raises(TypeError):
        gen.pairs([(0, 1)], [mm], ratio=0.5)
    # a capacity that is too small: the true offsets, the first `capacity` inliers
    cases = g["mixed"][0][10:16]
    flat = np.concatenate([c["matches"] for c in cases]); off = np.cumsum([0] + [len(c["matches"]) for c in cases])
    pairs = [(c["a"], c["b"]) for c in cases]
    full, foff, _ = gen.pairs_csr(pairs, flat, off, hypotheses=vc.H_SMALL)
    part, poff, _ = gen.pairs_csr(pairs, flat, off, capacity=37, hypotheses=vc.H_SMALL)
    assert foff[-1] == len(full) > 37 and len(part) == 37
    np.testing.assert_array_equal(poff, foff); np.testing.assert_array_equal(part, full[:37])
    none, noff, _ = gen.pairs_csr(pairs, flat, off, capacity=0, hypotheses=vc.H_SMALL)
    assert len(none) == 0 and noff[-1] == foff[-1]
    o = VF.verify_opts()
    assert (o.method, o.hypotheses, o.refine_rounds, o.min_inliers, o.max_error_px, o.seed) == (0, 1024, 2, 15, 4.0, 0)
    assert C.sizeof(L.VerifyOpts) == 32
    other = gen.pairs([(0, 1)], [mm], refine_rounds=0, seed=1)[1]                                     # another stream, a valid result
    assert other["status"][0] == VF.OK


def test_pipeline_verifies_the_matches_it_uses(pkg):
    """run_full_pipeline(verify_matches=True) on the small synthetic sequence with wrong matches injected into the caller's
    matches, each at least 20 px off its epipolar line under the true poses: they are gone from the matches the visual stage
    gets, the stage runs, and verify_matches=None is the run without the keyword bit for bit."""
    import test_gpu_mapq as tm
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    synth = importlib.import_module("global-lvba_amd.synth")
    d = tm._dataset()
    s = synth.make_scans(12, 40000, room=(14, 10, 4), n_panels=0, n_blobs=0, clutter_frac=0.0, seed=62, rot_sigma_deg=0.15, trans_sigma=0.04)
    Rcw, tcw = pipe.camera_from_imu(np.asarray(s["poses_gt"], np.float64).reshape(-1, 12), tm.RCB, tm.TCI)
    sc = dict(xy=[mo.undistort_all(tm.INTR, k) for k in d["kps"]], intr=tm.INTR, Rcw=Rcw, tcw=tcw)
    rng = np.random.default_rng(4)
    N_WRONG = 5
    matches, wrong = [], []
    for (a, b), m in zip(d["pairs"], d["matches"]):
        w = np.zeros((0, 2), np.int64)
        while len(w) < N_WRONG:
            cand = np.stack([rng.integers(0, len(d["kps"][a]), 64), rng.integers(0, len(d["kps"][b]), 64)], 1)
            dl, dh = vc.line_distances_px(sc, a, b, cand)
            w = np.vstack([w, cand[(dl >= vc.OUTLIER_PX) & (dh >= vc.OUTLIER_PX)]])
        w = w[:N_WRONG]
        mm = np.vstack([m, w])
        matches.append(mm[rng.permutation(len(mm))]); wrong.append({tuple(r) for r in w.tolist()} - {tuple(r) for r in m.tolist()})
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tm.RCB, tm.TCI, tm.INTR, tm.W, tm.H, d["kps"], d["pairs"])
    on = pipe.run_full_pipeline(*args, matches, verify_matches=True, **cfg)
    mv = on["match_verification"]
    assert mv["n_pairs"] == len(d["pairs"]) and len(on["matches"]) == len(d["pairs"]) and mv["n_pairs_ok"] > 0.5 * mv["n_pairs"]
    assert mv["n_matches"] == sum(len(m) for m in matches) and mv["n_inliers"] == sum(len(m) for m in on["matches"])
    kept_true = 0
    for m_out, m_in, w, rec in zip(on["matches"], d["matches"], wrong, mv["pairs"]):
        got = {tuple(r) for r in np.asarray(m_out).tolist()}
        assert not got & w                                   # every injected wrong match is gone
        assert rec["n_inliers"] == len(m_out) if rec["status"] == "ok" else len(m_out) == 0
        kept_true += len(got & {tuple(r) for r in m_in.tolist()})
    assert kept_true == mv["n_inliers"] and kept_true > 0.8 * sum(len(m) for m, r in zip(d["matches"], mv["pairs"]) if r["status"] == "ok")
    assert len(on["visual"]["landmarks"]) > 0 and np.isfinite(on["visual"]["Rcw"]).all()
    off = pipe.run_full_pipeline(*args, matches, verify_matches=None, **cfg)
    plain = pipe.run_full_pipeline(*args, matches, **cfg)
    assert "match_verification" not in off and "match_verification" not in plain
    assert off["poses"].tobytes() == plain["poses"].tobytes()
    for k in ("Rcw", "tcw", "landmarks", "landmark_valid", "track_status"):
        assert np.asarray(off["visual"][k]).tobytes() == np.asarray(plain["visual"][k]).tobytes(), k
