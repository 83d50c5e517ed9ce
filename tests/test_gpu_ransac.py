"""GPU test of the skeleton the two batched RANSAC stages share (csrc/ransac_device.h, csrc/ransac_batch.h; DESIGN.md §10k "The
skeleton"): the library against tests/golden/ransac_parent.npz, what the two stages returned on the same fixtures before the
skeleton was factored out of them (recorded by tests/golden/make_golden.py main_ransac on an MI355X).  Every array byte for byte,
the refined results included: the factoring changed no sum tree and no expression's order, and both files are built without
contraction."""
import importlib
import os

import numpy as np
import pytest

import resect_cases as rc
import verify_cases as vc
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_parent.npz")
ROUNDS = (0, 2)


def collect():
    """name -> array: lvba_verify_pairs on the mixed batch of each method and lvba_resect_images on the mixed batch of 40 jobs, each
    at refine_rounds 0 and 2 (every output array, inlier_off and the inlier lists); one lvba_verify_hypotheses call per method and
    one lvba_resect_hypotheses call at 65 elements and H = 65."""
    VF = importlib.import_module("global-lvba_amd.verify")
    RS = importlib.import_module("global-lvba_amd.resect")
    L = importlib.import_module("global-lvba_amd._lib")
    out = {}
    g = vc.general()
    sc = g["scene"]
    with VF.Verifier(sc["keypoints"], sc["intr"], Rcw=sc["Rcw"]) as v:
        for method in (0, 1):
            cases = g["mixed"][method]
            flat, off = L.flatten_rows([c["matches"] for c in cases], np.int32, 2)
            for rounds in ROUNDS:
                inl, ioff, rep = v.pairs_csr([(c["a"], c["b"]) for c in cases], flat, off, **dict(cases[0]["opts"], refine_rounds=rounds))
                for k in ("E", "status", "n_inliers", "best_h"):
                    out[f"verify_m{method}_r{rounds}_{k}"] = rep[k]
                out[f"verify_m{method}_r{rounds}_inlier_off"], out[f"verify_m{method}_r{rounds}_inliers"] = ioff, inl
            case, = [c for c in g["h_edges"] if c["opts"] == dict(method=method, hypotheses=65)]
            assert len(case["matches"]) == 65
            out[f"verify_m{method}_hyp_E"], out[f"verify_m{method}_hyp_count"] = v.hypotheses(case["a"], case["b"], case["matches"], **case["opts"])
    g = rc.general()
    cases = g["mixed"]
    assert len(cases) == 40
    intr = cases[0]["scene"]["intr"]
    uv, off = L.flatten_rows([c["uv"] for c in cases], np.float32, 2)
    world, _ = L.flatten_rows([c["world"] for c in cases], np.float64, 3)
    for rounds in ROUNDS:
        inl, ioff, rep = RS.resect_images_csr([c["id"] for c in cases], off, uv, world, intr, **dict(cases[0]["opts"], refine_rounds=rounds))
        for k in ("Rcw", "tcw", "status", "n_inliers", "best_h", "rmse_px", "information"):
            out[f"resect_r{rounds}_{k}"] = rep[k]
        out[f"resect_r{rounds}_inlier_off"], out[f"resect_r{rounds}_inliers"] = ioff, inl
    case, = [c for c in g["h_edges"] if c["opts"]["hypotheses"] == 65]
    assert len(case["uv"]) == 65
    out["resect_hyp_R"], out["resect_hyp_t"], out["resect_hyp_count"] = RS.hypotheses(case["id"], case["uv"], case["world"], intr, **case["opts"])
    return out


def test_both_stages_return_the_bytes_recorded_before_the_skeleton(pkg):
    want = np.load(GOLDEN)
    got = collect()
    assert sorted(got) == sorted(want.files)
    for k in sorted(got):
        w = want[k]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert np.ascontiguousarray(got[k]).tobytes() == w.tobytes(), k
    # the recording is of calls that did something: refits taken, tasks of every status but NO_MODEL, inliers written
    for m in (0, 1):
        assert (want[f"verify_m{m}_r2_n_inliers"] >= want[f"verify_m{m}_r0_n_inliers"]).all()
        assert set(want[f"verify_m{m}_r0_status"].tolist()) >= {0, 1} and len(want[f"verify_m{m}_r2_inliers"]) > 1000
        assert (want[f"verify_m{m}_hyp_count"] >= 0).sum() > 30
    assert (want["verify_m0_r2_E"] != want["verify_m0_r0_E"]).any() and (want["resect_r2_Rcw"] != want["resect_r0_Rcw"]).any()
    assert set(want["resect_r0_status"].tolist()) >= {0, 1} and len(want["resect_r2_inliers"]) > 1000 and (want["resect_hyp_count"] >= 0).sum() > 30
