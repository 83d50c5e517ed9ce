"""Times lvba_verify_pairs and lvba_verify_pairs_model: 10^3 and 10^4 image pairs at 100, 500 and 2 000 putative
matches each, both methods, the homography and the E-or-H choice (over method 0), 1024 hypotheses, best of 3 with the host clock around the call (upload, all kernels and download included).  For context, the
same host's time for the host emulation of the hypothesis stage (tests/verify_check.cpp) on a sample of pairs, scaled to the
batch.  No test runs this.

    python tools/verify_bench.py [--pairs 1000 10000] [--matches 100 500 2000] [--models essential homography auto] [--json out.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# fp64 instructions per (hypothesis, match) in the scoring loop of verify_hypothesis_kernel, counted in the gfx950 disassembly
# (18 v_mul_f64, 15 v_add_f64, 1 v_cmp); 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz
FP64_PER_EVAL = 34
# the same count for the homography's loop (24 v_mul_f64, 18 v_add_f64, 4 v_cmp: two transfers); "auto" is a run of each
FP64_PER_EVAL_H = 46
FP64_LANE_RATE = 256 * 4 * 16 * 2.4e9


def batch(sc, n_pairs, m, rng):
    """n_pairs pairs over the scene's four images with m matches each: 60 % planted, 40 % random"""
    import verify_cases as vc
    n_kp = vc.N_POINTS + vc.N_EXTRA
    pairs = np.array([vc.IMAGE_PAIRS[k % 6] for k in range(n_pairs)], np.int32)
    pts = rng.integers(0, vc.N_POINTS - 3, (n_pairs, m))
    mm = np.stack([pts, pts], -1)
    wrong = rng.random((n_pairs, m)) < 0.4
    mm[wrong] = rng.integers(0, n_kp, (int(wrong.sum()), 2))
    return pairs, np.ascontiguousarray(mm.reshape(-1, 2).astype(np.int32)), np.arange(n_pairs + 1, dtype=np.int64) * m


def host_emulation(sc, pairs, flat, off, method, sample=4):
    import match_oracle as mo
    import verify_oracle as vo
    so = os.path.join(tempfile.mkdtemp(), "libverify_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "verify_check.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    P_ = ctypes.c_void_p
    lib.emul_hypotheses.argtypes = [ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P_, P_,
                                    ctypes.c_double, P_, P_]
    t = 0.0
    for p in range(sample):
        a, b = int(pairs[p, 0]), int(pairs[p, 1])
        P = np.ascontiguousarray(vo.points(sc["xy"], a, b, flat[off[p]:off[p + 1]]))
        R = np.ascontiguousarray(vo.relative_rotation(sc["Rcw"][min(a, b)], sc["Rcw"][max(a, b)]))
        E, count = np.zeros((1024, 9)), np.zeros(1024, np.int32)
        t0 = time.perf_counter()
        lib.emul_hypotheses(method, 0, min(a, b), max(a, b), 1024, len(P), P.ctypes.data, R.ctypes.data, mo.tau2(sc["intr"], 4.0), E.ctypes.data,
                            count.ctypes.data)
        t += time.perf_counter() - t0
    return t / sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--matches", type=int, nargs="+", default=[100, 500, 2000])
    ap.add_argument("--models", nargs="+", default=["essential", "homography", "auto"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import verify_cases as vc
    VF = importlib.import_module("global-lvba_amd.verify")
    sc = vc.general()["scene"]
    rng = np.random.default_rng(0)
    rows = []
    with VF.Verifier(sc["keypoints"], sc["intr"], Rcw=sc["Rcw"]) as v:
        v.pairs_csr(*batch(sc, 8, 100, rng))                     # warm-up: module load, pools
        for n_pairs in a.pairs:
            for m in a.matches:
                pairs, flat, off = batch(sc, n_pairs, m, rng)
                runs = [("essential", 0), ("essential", 1), ("homography", 0), ("auto", 0)]
                for model, method in (r for r in runs if r[0] in a.models):
                    best = np.inf
                    for _ in range(3):
                        t0 = time.perf_counter()
                        _, ioff, rep = v.pairs_csr(pairs, flat, off, method=method, model=model)
                        best = min(best, time.perf_counter() - t0)
                    evals = n_pairs * 1024.0 * m
                    per = {"essential": FP64_PER_EVAL, "homography": FP64_PER_EVAL_H, "auto": FP64_PER_EVAL + FP64_PER_EVAL_H}[model]
                    bound = evals * per / FP64_LANE_RATE
                    host = host_emulation(sc, pairs, flat, off, method) * n_pairs if model == "essential" else None
                    row = dict(pairs=n_pairs, matches=m, model=model, method=method, seconds=best, bound_seconds=bound, share_of_bound=bound / best,
                               host_emulation_seconds=host, ok_pairs=int((rep["status"] == 0).sum()), inliers=int(ioff[-1]))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
