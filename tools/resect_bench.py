"""Times lvba_resect_images: 10^3 and 10^4 jobs at 100, 500 and 2 000 correspondences each, 1024 hypotheses, best
of 3 with the host clock around the call (upload, all kernels and download included).  For context, the same host's time for the
host emulation of the hypothesis stage (tests/resect_check.cpp) on a sample of jobs, scaled to the batch.  No test runs this.

    python tools/resect_bench.py [--jobs 1000 10000] [--corr 100 500 2000] [--json out.json]
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

# fp64 instructions per (hypothesis, correspondence) in the scoring loop of resect_hypothesis_kernel, counted in the gfx950
# disassembly (17 v_mul_f64, 12 v_add_f64, 2 v_cmp); 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz
FP64_PER_EVAL = 31
FP64_LANE_RATE = 256 * 4 * 16 * 2.4e9


def batch(sc, n_jobs, m, rng):
    """n_jobs jobs over the scene's four views with m correspondences each: 60 % planted, 40 % a keypoint with another point"""
    import verify_cases as vc
    view = np.arange(n_jobs) % 4
    pts = rng.integers(0, vc.N_POINTS - 3, (n_jobs, m))
    other = np.where(rng.random((n_jobs, m)) < 0.4, rng.integers(0, vc.N_POINTS - 3, (n_jobs, m)), pts)
    kps = np.stack([k[:vc.N_POINTS - 3] for k in sc["keypoints"]])            # [4, n, 2]
    uv = kps[view[:, None], pts].reshape(-1, 2).astype(np.float32)
    world = sc["X"][other].reshape(-1, 3)
    return np.arange(n_jobs, dtype=np.int32), np.arange(n_jobs + 1, dtype=np.int64) * m, np.ascontiguousarray(uv), np.ascontiguousarray(world)


def host_emulation(sc, off, uv, world, sample=4):
    import resect_oracle as ro
    so = os.path.join(tempfile.mkdtemp(), "libresect_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "resect_check.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    P_, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    lib.emul_hypotheses.argtypes = [ctypes.c_uint64, I, I, I, P_, D, D, D, P_, P_, P_]
    t = 0.0
    for j in range(sample):
        rec = np.ascontiguousarray(ro.records(sc["intr"], uv[off[j]:off[j + 1]], world[off[j]:off[j + 1]]))
        R, tt, count = np.zeros((1024, 9)), np.zeros((1024, 3)), np.zeros(1024, np.int32)
        t0 = time.perf_counter()
        lib.emul_hypotheses(0, j, 1024, len(rec), rec.ctypes.data, sc["intr"][0], sc["intr"][1], 8.0, R.ctypes.data, tt.ctypes.data, count.ctypes.data)
        t += time.perf_counter() - t0
    return t / sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--corr", type=int, nargs="+", default=[100, 500, 2000])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import verify_cases as vc
    RS = importlib.import_module("global-lvba_amd.resect")
    sc = vc.general()["scene"]
    rng = np.random.default_rng(0)
    rows = []
    RS.resect_images_csr(*batch(sc, 8, 100, rng), sc["intr"])                  # warm-up: module load, pools
    for n_jobs in a.jobs:
        for m in a.corr:
            ids, off, uv, world = batch(sc, n_jobs, m, rng)
            best = np.inf
            for _ in range(3):
                t0 = time.perf_counter()
                _, ioff, rep = RS.resect_images_csr(ids, off, uv, world, sc["intr"])
                best = min(best, time.perf_counter() - t0)
            evals = n_jobs * 1024.0 * m
            bound = evals * FP64_PER_EVAL / FP64_LANE_RATE
            host = host_emulation(sc, off, uv, world) * n_jobs
            row = dict(jobs=n_jobs, correspondences=m, seconds=best, bound_seconds=bound, share_of_bound=bound / best,
                       host_emulation_seconds=host, ok_jobs=int((rep["status"] == 0).sum()), inliers=int(ioff[-1]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
