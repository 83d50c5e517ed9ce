"""GPU tests of the homography model of the two-view verification and of the E-or-H choice (lvba_verify_pairs_model,
lvba_verify_hypotheses_homography, lvba_verify_score_homography, verify.Verifier's model keyword) against the numpy restatement
(tests/verify_h_oracle.py) on the shared fixtures (tests/verify_h_cases.py).  A hypothesis is formed from +, -,
*, / and sqrt in one order and the file is built without contraction: H, counts, winners, inlier lists and the choice are
compared exactly.  Only the refit, which goes through Jacobi, is held to the tolerance measured in test_verify_h_host.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import match_oracle as mo
import verify_cases as vc
import verify_h_cases as hc
import verify_h_oracle as ho
import verify_oracle as vo
from test_verify_h_host import REFIT_TOL

pytestmark = pytest.mark.gpu
MARGIN = 1e-9


@pytest.fixture(scope="module")
def VF(pkg):
    return importlib.import_module("global-lvba_amd.verify")


@pytest.fixture(scope="module")
def verifiers(VF):
    """scene -> Verifier, by the scene's seed"""
    scenes = [vc.general()["scene"], vc.planar()["scene"], hc.both(), hc.collinear_scene()]
    vs = {repr(sc["rng_seed"]): VF.Verifier(sc["keypoints"], sc["intr"], Rcw=sc["Rcw"]) for sc in scenes}
    yield lambda case: vs[repr(case["scene"]["rng_seed"])]
    for v in vs.values():
        v.close()


def run_batch(v, cases, **over):
    o = dict(cases[0]["opts"], **over)
    return v.pairs([(c["a"], c["b"]) for c in cases], [c["matches"] for c in cases], **o)


def check_batch_exact(got, rs, cases):
    ginl, rep = got
    np.testing.assert_array_equal(rep["status"], [r["status"] for r in rs])
    np.testing.assert_array_equal(rep["best_h"], [r["best_h"] for r in rs])
    np.testing.assert_array_equal(rep["n_inliers"], [r["n_inliers"] for r in rs])
    np.testing.assert_array_equal(rep["E"].reshape(-1, 9), np.array([r["E"] for r in rs]).reshape(-1, 9))
    for g, c, r in zip(ginl, cases, rs):
        np.testing.assert_array_equal(g, c["matches"][r["mask"]], err_msg=c["name"])


def mask_of(case, inl):
    """the inliers are a subsequence of the matches, in their order"""
    got = np.zeros(len(case["matches"]), bool)
    i = 0
    for r in inl.tolist():
        while case["matches"][i].tolist() != r:
            i += 1
        got[i] = True
        i += 1
    return got


def test_hypotheses_equal_the_oracle(verifiers):
    """every hypothesis's H and count, bit for bit: the match-count ladder either side of the sample size, of the wavefront and of
    the LDS chunk, H either side of the hypothesis block, NaN keypoints, one match repeated, three points on a line, the claims,
    the mixed batch's pairs"""
    invalid = 0
    for case in hc.all_cases():
        Hm, count, _, _ = hc.oracle_hypotheses(case)
        gH, gcount = verifiers(case).hypotheses(case["a"], case["b"], case["matches"], model="homography", **case["opts"])
        np.testing.assert_array_equal(gH.reshape(-1, 9), Hm, err_msg=case["name"])
        np.testing.assert_array_equal(gcount, count, err_msg=case["name"])
        invalid += int((count == -1).sum())
    assert invalid > 0


def test_pairs_without_refinement_equal_the_oracle(verifiers, VF):
    c = hc.cases()
    cases = c["mixed"]
    v = verifiers(cases[0])
    rs = [hc.oracle_pair(k, refine_rounds=0) for k in cases]
    got = run_batch(v, cases, model="homography", refine_rounds=0)
    check_batch_exact(got, rs, cases)
    assert set(got[1]["status"].tolist()) >= {VF.OK, VF.TOO_FEW_MATCHES}
    assert (got[1]["kind"] == 1).all() and (got[1]["n_inliers_E"] == -1).all()
    np.testing.assert_array_equal(got[1]["n_inliers_H"], got[1]["n_inliers"])
    # two identical calls, the pairs one at a time, and the batch reversed: the same bytes
    again = run_batch(v, cases, model="homography", refine_rounds=0)
    back = run_batch(v, cases[::-1], model="homography", refine_rounds=0)
    for k in ("E", "status", "n_inliers", "best_h"):
        assert got[1][k].tobytes() == again[1][k].tobytes() and got[1][k].tobytes() == back[1][k][::-1].tobytes(), k
    for a, b, d in zip(got[0], again[0], back[0][::-1]):
        assert a.tobytes() == b.tobytes() == d.tobytes()
    for k in (0, 3, 7, 9, 17):
        one = run_batch(v, cases[k:k + 1], model="homography", refine_rounds=0)
        assert one[0][0].tobytes() == got[0][k].tobytes() and one[1]["E"][0].tobytes() == got[1]["E"][k].tobytes()
        assert one[1]["best_h"][0] == got[1]["best_h"][k]
    inl, rep = v.pairs(np.zeros((0, 2), np.int32), [], model="homography")
    assert inl == [] and len(rep["status"]) == 0 and len(rep["kind"]) == 0
    for case in c["sizes"] + c["h_edges"] + c["special"] + c["collinear"]:
        for over in (dict(), dict(min_inliers=0)):
            check_batch_exact(run_batch(verifiers(case), [case], model="homography", refine_rounds=0, **over),
                              [hc.oracle_pair(case, refine_rounds=0, **over)], [case])
    for case in c["special"] + c["collinear"]:
        inl, rep = run_batch(verifiers(case), [case], model="homography", min_inliers=0)
        assert rep["status"][0] == VF.NO_MODEL and rep["best_h"][0] == -1 and not rep["E"].any() and len(inl[0]) == 0
    # (hi, lo) is (lo, hi) with the columns swapped back
    (i0, r0), (i1, r1) = (run_batch(verifiers(k), [k], model="homography") for k in c["flipped"])
    assert r0["E"].tobytes() == r1["E"].tobytes() and r0["best_h"][0] == r1["best_h"][0]
    np.testing.assert_array_equal(i0[0], i1[0][:, ::-1])
    assert len(i0[0]) >= 15


def check_refined(v, cases, planted_claim):
    base_inl, base = run_batch(v, cases, model="homography", refine_rounds=0)
    inl, rep = run_batch(v, cases, model="homography")
    excluded = total = 0
    for k, case in enumerate(cases):
        P = hc.case_points(case)
        tau2 = mo.tau2(case["scene"]["intr"], 4.0)
        assert rep["n_inliers"][k] >= base["n_inliers"][k] and rep["best_h"][k] == base["best_h"][k]
        if rep["status"][k] != vo.OK:
            assert len(inl[k]) == 0
            continue
        want, rel = ho.score(rep["E"][k].reshape(9), P, tau2, with_margin=True)
        got = mask_of(case, inl[k])
        sure = rel > MARGIN
        np.testing.assert_array_equal(got[sure], want[sure], err_msg=case["name"])
        excluded += int((~sure).sum()); total += len(P)
        assert rep["n_inliers"][k] == got.sum()
        r = hc.oracle_pair(case)
        if r["n_inliers"] >= 30:
            d = float(np.abs(rep["E"][k].reshape(9) - r["E"]).max())
            print(case["name"], "refined H against the oracle's:", d)
            assert d <= REFIT_TOL, (case["name"], d)
        if planted_claim:
            np.testing.assert_array_equal(got, case["planted"], err_msg=case["name"])
    assert excluded <= 0.01 * total, (excluded, total)


def test_pairs_with_refinement(verifiers):
    c = hc.cases()
    for scene_cases in (c["planar_claims"][:1] + c["planar_claims"][2:], c["planar_claims"][1:2]):       # pairs (2, 3) and (0, 1)
        check_refined(verifiers(scene_cases[0]), scene_cases, True)
    check_refined(verifiers(c["mixed"][0]), c["mixed"], False)
    # the refit where it is taken: planar-80%'s winner misses planted matches and the refit finds them
    case = c["planar_claims"][3]
    r0, r = hc.oracle_pair(case, refine_rounds=0), hc.oracle_pair(case)
    inl, rep = run_batch(verifiers(case), [case], model="homography")
    assert r["n_inliers"] > r0["n_inliers"] and rep["n_inliers"][0] == r["n_inliers"] and rep["best_h"][0] == r["best_h"]


def raw_pairs_model(v, L, cases, model, planar_ratio=0.8, capacity=None, with_counts=True, **opts):
    """lvba_verify_pairs_model as it is: dict of its outputs"""
    VF = importlib.import_module("global-lvba_amd.verify")
    pairs = np.ascontiguousarray([(k["a"], k["b"]) for k in cases], np.int32).reshape(-1, 2)
    flat, off = L.flatten_rows([k["matches"] for k in cases], np.int32, 2)
    P = len(pairs)
    cap = len(flat) if capacity is None else capacity
    o = VF.verify_opts(v.lib, **opts)
    out = dict(inliers=np.zeros((cap, 2), np.int32), off=np.zeros(P + 1, np.int64), M=np.zeros((P, 9)),
               **{k: np.full(P, -7, np.int32) for k in ("kind", "status", "n_inliers", "best_h", "n_E", "n_H")})
    p = lambda a: a.ctypes.data
    rc = v.lib.lvba_verify_pairs_model(v._h, P, p(pairs), p(off), p(flat), C.byref(o), model, planar_ratio, cap, p(out["off"]), p(out["inliers"]),
                                       p(out["M"]), p(out["kind"]), p(out["status"]), p(out["n_inliers"]), p(out["best_h"]),
                                       p(out["n_E"]) if with_counts else None, p(out["n_H"]) if with_counts else None)
    out["rc"] = rc
    return out


def test_auto_chooses_per_pair(verifiers, VF, pkg):
    L = pkg._lib
    c = hc.cases()
    cases = c["mixed"]
    v = verifiers(cases[0])
    pairs, ms = [(k["a"], k["b"]) for k in cases], [k["matches"] for k in cases]
    # without refinement every figure is exact: kind and both counts against the oracle
    inl, rep = v.pairs(pairs, ms, model="auto", method=0, hypotheses=hc.H_SMALL, refine_rounds=0)
    want = [hc.oracle_auto(k, refine_rounds=0) for k in cases]
    np.testing.assert_array_equal(rep["kind"], [r["kind"] for r in want])
    np.testing.assert_array_equal(rep["n_inliers_E"], [r["n_inliers_E"] for r in want])
    np.testing.assert_array_equal(rep["n_inliers_H"], [r["n_inliers_H"] for r in want])
    check_batch_exact((inl, rep), want, cases)
    assert set(rep["kind"].tolist()) == {0, 1}
    # with refinement: the ESSENTIAL pairs' outputs are lvba_verify_pairs' bytes, the HOMOGRAPHY pairs' the homography call's
    inl, rep = v.pairs(pairs, ms, model="auto", method=0, hypotheses=hc.H_SMALL)
    iE, rE = v.pairs(pairs, ms, method=0, hypotheses=hc.H_SMALL)
    iH, rH = v.pairs(pairs, ms, model="homography", hypotheses=hc.H_SMALL)
    assert set(rep["kind"].tolist()) == {0, 1}
    for k, case in enumerate(cases):
        src_i, src = (iH, rH) if rep["kind"][k] == 1 else (iE, rE)
        for f in ("E", "status", "n_inliers", "best_h"):
            assert rep[f][k].tobytes() == src[f][k].tobytes(), (case["name"], f)
        assert inl[k].tobytes() == src_i[k].tobytes(), case["name"]
        assert rep["n_inliers_E"][k] == rE["n_inliers"][k] and rep["n_inliers_H"][k] == rH["n_inliers"][k]
        assert rep["kind"][k] == ho.choose(dict(status=rE["status"][k], n_inliers=rE["n_inliers"][k]),
                                           dict(status=rH["status"][k], n_inliers=rH["n_inliers"][k]))
        if len(case["matches"]) >= 60:
            assert rep["kind"][k] == (1 if case["planar"] else 0), case["name"]
    # planar_ratio moves the choice: far above every ratio nothing is a plane unless E fails; far below, everything H accepts is
    hi = v.pairs(pairs, ms, model="auto", method=0, hypotheses=hc.H_SMALL, planar_ratio=100.0)[1]
    lo = v.pairs(pairs, ms, model="auto", method=0, hypotheses=hc.H_SMALL, planar_ratio=1e-6)[1]
    np.testing.assert_array_equal(hi["kind"] == 1, (rH["status"] == VF.OK) & (rE["status"] != VF.OK))
    np.testing.assert_array_equal(lo["kind"] == 1, rH["status"] == VF.OK)
    # model = essential through the new entry point is lvba_verify_pairs, byte for byte; both count arrays may be NULL
    for with_counts in (True, False):
        raw = raw_pairs_model(v, L, cases, 0, with_counts=with_counts, method=0, hypotheses=hc.H_SMALL)
        assert raw["rc"] == 0
        flat_E = np.concatenate(iE) if len(iE) else np.zeros((0, 2), np.int32)
        assert raw["M"].tobytes() == rE["E"].tobytes() and raw["inliers"][:raw["off"][-1]].tobytes() == flat_E.tobytes()
        for f in ("status", "n_inliers", "best_h"):
            assert raw[f].tobytes() == rE[f].tobytes(), f
        assert (raw["kind"] == 0).all()
        if with_counts:
            assert raw["n_E"].tobytes() == rE["n_inliers"].tobytes() and (raw["n_H"] == -1).all()
        else:
            assert (raw["n_E"] == -7).all() and (raw["n_H"] == -7).all()
    # the rotation-aided method as the E side of the choice
    r1 = v.pairs(pairs, ms, model="auto", method=1, hypotheses=hc.H_SMALL)[1]
    e1 = v.pairs(pairs, ms, method=1, hypotheses=hc.H_SMALL)[1]
    np.testing.assert_array_equal(r1["n_inliers_E"], e1["n_inliers"])
    np.testing.assert_array_equal(r1["n_inliers_H"], rH["n_inliers"])


def test_auto_on_the_claims(verifiers):
    """default options: HOMOGRAPHY on every planar case, ESSENTIAL on every general one, exactly the planted set on all, and the
    oracle's counts"""
    c = hc.cases()
    for cases in (c["planar_claims"][:1] + c["planar_claims"][2:], c["planar_claims"][1:2], c["general_claims"][:1], c["general_claims"][1:]):
        inl, rep = run_batch(verifiers(cases[0]), cases, model="auto", method=0)
        for k, case in enumerate(cases):
            r = hc.oracle_auto(case)
            assert rep["kind"][k] == r["kind"] == (1 if case["name"].startswith("planar") else 0), case["name"]
            assert rep["status"][k] == vo.OK
            np.testing.assert_array_equal(mask_of(case, inl[k]), case["planted"], err_msg=case["name"])
            assert (rep["n_inliers_E"][k], rep["n_inliers_H"][k]) == (r["n_inliers_E"], r["n_inliers_H"]), case["name"]


def test_score_homography_is_the_oracles_gate(verifiers):
    c = hc.cases()
    for case in c["planar_claims"] + c["general_claims"]:
        v = verifiers(case)
        Hm, count, _, _ = hc.oracle_hypotheses(case)
        P = hc.case_points(case)
        for M in (Hm[vo.pick(count)[0]], hc.oracle_pair(case)["E"]):
            for px in (4.0, 1.0):
                want, rel = ho.score(M, P, mo.tau2(case["scene"]["intr"], px), with_margin=True)
                got = v.score_homography(case["a"], case["b"], case["matches"], M, max_error_px=px)
                np.testing.assert_array_equal(got[rel > MARGIN], want[rel > MARGIN], err_msg=case["name"])
                assert (rel > MARGIN).mean() > 0.99
        if case["name"].startswith("planar"):
            fin = ~np.isnan(P).any(axis=1)
            assert v.score_homography(case["a"], case["b"], case["matches"], hc.oracle_pair(case)["E"])[case["planted"] & fin].all()
        for M in (np.zeros(9), np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1]), np.full(9, np.nan)):          # no inverse direction: nothing passes
            assert not v.score_homography(case["a"], case["b"], case["matches"], M).any()


def test_error_paths(VF, verifiers, pkg):
    L = pkg._lib
    c = hc.cases()
    case = c["planar_claims"][1]
    v = verifiers(case)
    mm = case["matches"]
    sc = case["scene"]
    for kw in (dict(model=3), dict(model=-1), dict(model="auto", planar_ratio=0.0), dict(model="auto", planar_ratio=-0.8),
               dict(model="auto", planar_ratio=float("nan")), dict(model="auto", planar_ratio=float("inf")),
               dict(model="homography", planar_ratio=0.0), dict(model="auto", method=2), dict(model="auto", hypotheses=0),
               dict(model="homography", max_error_px=0.0), dict(model="homography", hypotheses=0)):
        with pytest.raises(L.LvbaError) as e:
            v.pairs([(0, 1)], [mm], **kw)
        assert e.value.code == L.ERR_ARG, kw
    bad = mm.copy(); bad[7, 1] = len(sc["keypoints"][1])
    for pairs, ms in (([(0, 0)], [mm]), ([(0, 4)], [mm]), ([(0, 1)], [bad])):
        for model in ("homography", "auto"):
            with pytest.raises(L.LvbaError) as e:
                v.pairs(pairs, ms, model=model)
            assert e.value.code == L.ERR_ARG
    with pytest.raises(L.LvbaError):
        v.hypotheses(0, 1, bad, model="homography")
    with pytest.raises(L.LvbaError):
        v.score_homography(1, 1, mm, np.eye(3))
    with pytest.raises(L.LvbaError):
        v.score_homography(0, 1, mm, np.eye(3), max_error_px=-1.0)
    with VF.Verifier(sc["keypoints"], sc["intr"]) as bare:             # no rotations
        with pytest.raises(L.LvbaError) as e:
            bare.pairs([(0, 1)], [mm], model="auto", method=1)
        assert e.value.code == L.ERR_ARG and "Rcw" in str(e.value)
        got = bare.pairs([(0, 1)], [mm], model="homography", method=1, refine_rounds=0)[1]        # the homography reads no method
        assert got["E"].tobytes() == v.pairs([(0, 1)], [mm], model="homography", refine_rounds=0)[1]["E"].tobytes()
    # a null kind is refused; the old entry point still refuses method 2 and lvba_verify_opts is still 32 bytes
    pairs = np.array([[0, 1]], np.int32); off = np.array([0, len(mm)], np.int64); ioff = np.zeros(2, np.int64)
    inl = np.zeros((len(mm), 2), np.int32); M = np.zeros(9); st, n, h = (np.zeros(1, np.int32) for _ in range(3))
    o = VF.verify_opts(v.lib)
    rc = v.lib.lvba_verify_pairs_model(v._h, 1, pairs.ctypes.data, off.ctypes.data, mm.ctypes.data, C.byref(o), 2, 0.8, len(mm), ioff.ctypes.data,
                                       inl.ctypes.data, M.ctypes.data, None, st.ctypes.data, n.ctypes.data, h.ctypes.data, None, None)
    assert rc == L.ERR_ARG
    with pytest.raises(L.LvbaError):
        v.pairs([(0, 1)], [mm], method=2)
    assert C.sizeof(L.VerifyOpts) == 32
    # a capacity that is too small: the true offsets, the first `capacity` inliers, under either new model
    cases = c["mixed"][10:16]
    bv = verifiers(cases[0])
    flat = np.concatenate([k["matches"] for k in cases]); moff = np.cumsum([0] + [len(k["matches"]) for k in cases])
    pairs = [(k["a"], k["b"]) for k in cases]
    for model in ("homography", "auto"):
        full, foff, _ = bv.pairs_csr(pairs, flat, moff, hypotheses=hc.H_SMALL, model=model, method=0)
        part, poff, _ = bv.pairs_csr(pairs, flat, moff, capacity=37, hypotheses=hc.H_SMALL, model=model, method=0)
        assert foff[-1] == len(full) > 37 and len(part) == 37
        np.testing.assert_array_equal(poff, foff); np.testing.assert_array_equal(part, full[:37])
        none, noff, _ = bv.pairs_csr(pairs, flat, moff, capacity=0, hypotheses=hc.H_SMALL, model=model, method=0)
        assert len(none) == 0 and noff[-1] == foff[-1]


def test_pipeline_hands_the_model_on(pkg):
    """run_full_pipeline(verify_matches=dict(model="auto")) on the small synthetic sequence: plumbing only -- the report's new
    fields, and every match that is kept is one that was given.  No claim on the room's wrong matches."""
    import test_gpu_mapq as tm
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = tm._dataset()
    cfg = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tm.RCB, tm.TCI, tm.INTR, tm.W, tm.H, d["kps"], d["pairs"])
    on = pipe.run_full_pipeline(*args, d["matches"], verify_matches=dict(model="auto"), **cfg)
    mv = on["match_verification"]
    assert mv["n_pairs"] == len(d["pairs"]) == len(on["matches"]) and 0 <= mv["n_pairs_planar"] <= mv["n_pairs_ok"]
    planar = 0
    for m_out, m_in, rec in zip(on["matches"], d["matches"], mv["pairs"]):
        assert rec["model"] in ("essential", "homography") and rec["n_inliers_E"] >= 0 and rec["n_inliers_H"] >= 0
        assert rec["n_inliers"] == (rec["n_inliers_H"] if rec["model"] == "homography" else rec["n_inliers_E"])
        assert {tuple(r) for r in np.asarray(m_out).tolist()} <= {tuple(r) for r in np.asarray(m_in).tolist()}
        assert len(m_out) == (rec["n_inliers"] if rec["status"] == "ok" else 0)
        planar += rec["status"] == "ok" and rec["model"] == "homography"
    assert planar == mv["n_pairs_planar"] and mv["n_inliers"] == sum(len(m) for m in on["matches"])
