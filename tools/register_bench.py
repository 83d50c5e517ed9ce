"""Scan-to-map registration throughput (lvba_register_scans): 64 jobs of 100 k points against the plane map of 64 frames.

    python tools/register_bench.py [--jobs 64] [--points 100000] [--iterations 20] [--repeat 5]

Prints one JSON line: ms per call and per Gauss-Newton iteration (host clock around calls that end in a device synchronise;
tolerances 0, so every job takes exactly --iterations linearisations), points per second, and the algorithmic bytes of an
iteration -- 12 B per point (the fp32 coordinates; the map tables are a few hundred KB and stay in L2) -- over that time.
Kernel split: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/register_bench.py --repeat 1`
(reg_linearize_kernel, reg_step_kernel), in a run of its own.  Needs a HIP device."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("global-lvba_amd")
    synth = importlib.import_module("global-lvba_amd.synth")
    reg = importlib.import_module("global-lvba_amd.register")
    if pkg._lib.load().lvba_device_count() < 1:
        raise SystemExit("register_bench needs a HIP device")
    s = synth.make_scans(a.jobs, a.points, seed=5, noise=0.005, clutter_frac=0.05)
    sc = pkg.Scans(s["clouds"])
    frames = np.arange(a.jobs, dtype=np.int32)
    opts = dict(max_iterations=a.iterations, tol_rot=0.0, tol_pos=0.0)
    with sc.voxel_map(s["poses_gt"], 1.0, reg.STRICT_RATIO) as m:
        r = m.register(sc, frames, s["poses"], **opts)                       # warm-up: code objects, pools
        ms = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            r = m.register(sc, frames, s["poses"], **opts)
            ms.append(1e3 * (time.perf_counter() - t0))
        info = dict(m.info)
    iters = int(r["iterations"].sum())
    pts = int(r["points"].sum())
    best = min(ms)
    per_it = best / a.iterations
    print(json.dumps(dict(bench="register", jobs=a.jobs, points_per_job=a.points, map_roots=info["n_roots"], map_planes=info["n_planes"],
                          iterations=a.iterations, iterations_taken=iters, status=sorted(set(r["status_name"])),
                          inliers_mean=float(r["inliers"].mean()), call_ms=[round(v, 3) for v in ms], ms_per_iteration=round(per_it, 4),
                          points_per_s=pts / (per_it * 1e-3), algorithmic_GBps=12.0 * pts / (per_it * 1e-3) / 1e9)))
    sc.close()


if __name__ == "__main__":
    main()
