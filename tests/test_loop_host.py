"""CPU tests of the loop-closure detection: the device header of the candidate search (csrc/loop_device.h) compiled for the host
against the numpy restatement (tests/loop_oracle.py), the conditions on the shared fixture (tests/loop_cases.py, DESIGN.md
§10d), the acceptance rule, the shared prior helper and the struct layouts."""
import ctypes
import importlib

import numpy as np
import pytest

from host_build import build_check

import loop_cases as lc
import loop_oracle as lo
import register_oracle as ro


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("loop_check", tmp_path_factory.mktemp("emul_loop")))
    f64 = np.ctypeslib.ndpointer(np.float64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    lib.emul_candidates.argtypes = [ctypes.c_int, f64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                    ctypes.c_int64, i32, i32, i32, f64]
    lib.emul_candidates.restype = ctypes.c_int64
    return lib


def host_candidates(emul, poses, submap_size=10, min_gap=50, max_per_frame=2, query_stride=1, radius=5.0):
    pos = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12)[:, 9:])
    cap = max(1, len(pos) * max_per_frame)
    q, w, r, d = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
    n = emul.emul_candidates(len(pos), pos if len(pos) else np.zeros((1, 3)), submap_size, min_gap, max_per_frame, query_stride, radius,
                             cap, q, w, r, d)
    return [(int(q[k]), int(w[k]), int(r[k]), float(d[k])) for k in range(n)]


def search_cases():
    """(name, poses, options): every candidate search the tests run."""
    P = lc.truth()
    out = [("fixture", P, lc.SEARCH), ("drifted", lc.drifted(), lc.SEARCH),
           ("max_per_frame=1", P, dict(lc.SEARCH, max_per_frame=1, radius=lc.RADIUS_WIDE)),
           ("wide", P, dict(lc.SEARCH, radius=lc.RADIUS_WIDE)),
           ("query_stride=2", P, dict(lc.SEARCH, query_stride=2)),
           ("min_gap=8", P, dict(lc.SEARCH, min_gap=8)), ("min_gap=9", P, dict(lc.SEARCH, min_gap=9)),
           ("n < submap_size", P[:2], dict(lc.SEARCH, submap_size=3, min_gap=1, radius=10.0)),
           ("n = 0", P[:0], lc.SEARCH)]
    # a submap of exactly one wavefront of frames, and of one frame more, each followed by a last submap of a single frame
    ragged = dict(submap_size=64, min_gap=0, max_per_frame=2, query_stride=1, radius=3.0)
    out += [("64 + 1 frames", lc.laps()[:65], ragged), ("65 + 1 frames", lc.laps()[:66], dict(ragged, submap_size=65))]
    return out + [(f"laps {k}", lc.laps(), o) for k, o in enumerate(lc.LAPS_CASES)]


def test_host_candidates_match_oracle(emul):
    """The header's rule, query by query, against numpy: the same lists, distances bit for bit."""
    for name, P, o in search_cases():
        assert host_candidates(emul, P, **o) == lo.candidates(P, **o), name
    for j, f0, f1, g in ((5, 0, 3, 3), (5, 0, 3, 4), (0, 6, 9, 6), (0, 6, 9, 7), (4, 3, 6, 0), (4, 3, 6, 1)):
        assert bool(emul.emul_gap_ok(j, f0, f1, g)) == all(abs(j - f) >= g for f in range(f0, f1))


def test_fixture_candidates_cover_every_clause():
    """Each clause of the rule has a pair it admits and a pair it rejects, and every decision has a margin >= 1e-9 relative."""
    P = lc.truth()
    pr = lo.pairs(P, lc.S, lc.MIN_GAP, lc.RADIUS)
    assert any(p["gap_ok"] for p in pr) and any(not p["gap_ok"] and p["radius_ok"] for p in pr)              # gap
    assert any(p["gap_ok"] and p["radius_ok"] for p in pr) and any(p["gap_ok"] and not p["radius_ok"] for p in pr)   # radius
    assert lc.candidates("truth") == [(0, 3, 11, pytest.approx(0.99, abs=0.01)), (1, 3, 11, pytest.approx(1.87, abs=0.01)),
                                      (10, 0, 0, pytest.approx(1.98, abs=0.01)), (11, 0, 0, pytest.approx(0.99, abs=0.01))]
    wide = lo.candidates(P, **dict(lc.SEARCH, radius=lc.RADIUS_WIDE))
    cut = lo.candidates(P, **dict(lc.SEARCH, radius=lc.RADIUS_WIDE, max_per_frame=1))
    assert set(cut) < set(wide) and (11, 0) in {c[:2] for c in cut} and (11, 1) in {c[:2] for c in set(wide) - set(cut)}   # truncation
    strided = lo.candidates(P, **dict(lc.SEARCH, query_stride=2))
    assert {c[0] for c in strided} == {0, 10} and {c[0] for c in lc.candidates("truth")} - {c[0] for c in strided} == {1, 11}   # stride
    assert len(lo.candidates(P, **dict(lc.SEARCH, min_gap=8))) == 4 and len(lo.candidates(P, **dict(lc.SEARCH, min_gap=9))) == 2
    for which in ("truth", "drifted"):
        for r in (lc.RADIUS, lc.RADIUS_WIDE):
            assert lo.decision_margin(lc.poses(which), lc.S, lc.MIN_GAP, r) >= 1e-9
    # the laps case has what the fixture cannot: exact ties and queries with more eligible submaps than are kept
    L0 = lc.LAPS_CASES[0]
    el = [p for p in lo.pairs(lc.laps(), L0["submap_size"], L0["min_gap"], L0["radius"]) if p["gap_ok"] and p["radius_ok"]]
    per_query = {}
    for p in el:
        per_query.setdefault(p["query"], []).append(p["d2"])
    assert any(len(v) > L0["max_per_frame"] for v in per_query.values()) and any(len(set(v)) < len(v) for v in per_query.values())
    # the ragged cases have candidates in the full submap and in the last one of a single frame
    for name, P, o in search_cases():
        if name.endswith("+ 1 frames"):
            assert {c[1] for c in lo.candidates(P, **o)} == {0, 1} and len(P) == o["submap_size"] + 1


def test_fixture_registrations_meet_their_conditions():
    """At the true poses every candidate registers with rmse < 3 x noise and >= 1000 inliers; from the drifted poses the oracle
    converges for every candidate it accepts; association and gate margins >= 1e-9 m on every linearisation."""
    for q, w, ref, d in lc.candidates("truth"):
        reg = lc.oracle_register("truth", q, w)
        assert reg["status"] == ro.CONVERGED and reg["rmse"] < 3 * lc.NOISE and reg["inliers"] >= 1000
        assert min(t["margin"] for t in reg["trace"]) >= 1e-9
    accepted = 0
    for q, w, ref, d in lc.candidates("drifted"):
        ok, why, reg = lc.oracle_accept("drifted", q, w)
        assert min(t["margin"] for t in reg["trace"]) >= 1e-9
        if ok:
            accepted += 1
            assert reg["status"] == ro.CONVERGED
    assert accepted >= 2


def test_acceptance_rule_reasons():
    pl = importlib.import_module("global-lvba_amd.pipeline")
    base = dict(status=0, inliers=1500, points=3000, rmse=0.01, rot=0.01, trans=0.05)
    bounds = dict(min_inlier_frac=0.3, max_rmse=0.03, max_rot=0.05, max_trans=0.2)
    for change, why in (({}, None), (dict(status=1), "status"), (dict(status=2), "status"), (dict(inliers=899), "inliers"),
                        (dict(inliers=900), None), (dict(rmse=0.031), "rmse"), (dict(rot=0.06), "correction"), (dict(trans=0.3), "correction"),
                        (dict(status=3, inliers=0, rmse=1.0), "status"), (dict(inliers=0, rmse=1.0), "inliers")):
        a = dict(base)
        a.update(change)
        for f in (pl.loop_acceptance, lo.accept):
            assert f(a["status"], a["inliers"], a["points"], a["rmse"], a["rot"], a["trans"], **bounds) == (why is None, why)
    # bounds that are not given do not bind
    assert pl.loop_acceptance(0, 1500, 3000, 9.0, 3.0, 9.0) == (True, None)
    T0, T = lc.truth()[0], ro.retract(lc.truth()[0], np.r_[0.0, 0.0, 0.02, 0.3, 0.0, 0.4])
    assert np.allclose(pl.pose_correction(T0, T), (0.02, 0.5), atol=1e-12) and pl.pose_correction(T0, T) == lo.correction(T0, T)


def test_shared_prior_helper_is_loop_closure_priors_arithmetic():
    """registration_prior on a recorded registration: the measurement T_i^-1 T_j and the upper Cholesky factor of
    M H M^T / sigma^2, operation for operation what loop_closure_prior computed before the helper existed."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    q, w, ref, _ = lc.candidates("drifted")[0]
    reg = lc.oracle_register("drifted", q, w)
    x = lc.drifted()
    for sigma in (None, 0.02):
        pr = pl.registration_prior(ref, q, x[ref], reg["pose"], reg["information"], reg["rmse"], reg["status"], sigma)
        Ri, pi = x[ref, :9].reshape(3, 3), x[ref, 9:]
        Tj = reg["pose"]
        meas = np.r_[(Ri.T @ Tj[:9].reshape(3, 3)).reshape(9), Ri.T @ (Tj[9:] - pi)]
        s2 = float(reg["rmse"]) ** 2 if sigma is None else float(sigma) ** 2
        M = np.zeros((6, 6))
        M[:3, :3], M[3:, 3:] = np.eye(3), Ri.T
        want = np.linalg.cholesky(M @ reg["information"] @ M.T / s2).T
        assert pr.kind == 2 and pr.i == ref and pr.j == q
        assert np.array_equal(np.array(pr.meas[:]), meas) and np.array_equal(np.array(pr.sqrt_info[:]).reshape(6, 6), want)
    dead = pl.registration_prior(ref, q, x[ref], reg["pose"], reg["information"], reg["rmse"], ro.DEGENERATE)
    assert not np.any(np.array(dead.sqrt_info[:]))


def test_loop_struct_sizes_match_the_header():
    L = importlib.import_module("global-lvba_amd._lib")
    # the layout of lvba_loop_opts / lvba_loop_candidate against the header: tests/test_abi.py, every struct at once
    new = ("lvba_submaps_build", "lvba_submaps_count", "lvba_submaps_find_planes", "lvba_register_linearize_submaps",
           "lvba_register_scans_submaps", "lvba_loop_default_opts", "lvba_loop_candidates")
    assert all(s in L.SYMBOLS for s in new)
    # tests/test_gpu_register.py finds two internal builders by substring over the exported names: no public name may hold either
    assert not any("lvba_voxmap_build_scans_joint" in s or "lvba_voxmap_window_view" in s for s in L.SYMBOLS)
