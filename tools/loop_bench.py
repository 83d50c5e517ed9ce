"""Loop-closure detection timings: the candidate search (lvba_loop_candidates) on a synthetic multi-lap trajectory, and the
submap path of the registration (lvba_submaps_build, lvba_register_scans_submaps) against the single-map path on
tools/register_bench.py's workload.

    python tools/loop_bench.py [--frames 2000 10000] [--jobs 64] [--points 100000] [--iterations 20] [--repeat 5]

Prints one JSON line (host clock around calls that end in a device synchronise, best of --repeat).  Needs a HIP device."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best_ms(fn, repeat):
    fn()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(min(ms), 3)


def trajectory(n):
    """Laps of 500 frames on a circle of radius 40 m, 1 m apart in height: every frame revisits every other lap."""
    t = np.arange(n) * (2 * np.pi / 500)
    P = np.zeros((n, 12))
    P[:, :9] = np.eye(3).reshape(9)
    P[:, 9], P[:, 10], P[:, 11] = 40 * np.cos(t), 40 * np.sin(t), np.arange(n) // 500
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[2000, 10000])
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("global-lvba_amd")
    synth = importlib.import_module("global-lvba_amd.synth")
    reg = importlib.import_module("global-lvba_amd.register")
    if pkg._lib.load().lvba_device_count() < 1:
        raise SystemExit("loop_bench needs a HIP device")
    out = dict(bench="loop", candidates=[])
    for n in a.frames:
        P = trajectory(n)
        got = reg.loop_candidates(P)
        out["candidates"].append(dict(frames=n, count=got["count"], ms=best_ms(lambda: reg.loop_candidates(P), a.repeat)))
    if a.jobs > 0:
        s = synth.make_scans(a.jobs, a.points, seed=5, noise=0.005, clutter_frac=0.05)
        frames = np.arange(a.jobs, dtype=np.int32)
        opts = dict(max_iterations=a.iterations, tol_rot=0.0, tol_pos=0.0)
        with pkg.Scans(s["clouds"]) as sc:
            def separate():
                for f in range(a.jobs):
                    sc.voxel_map(s["poses_gt"][f:f + 1], 1.0, reg.STRICT_RATIO, frame_begin=f, n_frames=1).close()
            out["build_submaps_ms"] = best_ms(lambda: sc.submaps(s["poses_gt"], 1, 1.0, reg.STRICT_RATIO).close(), a.repeat)
            out["build_separate_ms"] = best_ms(separate, a.repeat)
            with sc.voxel_map(s["poses_gt"], 1.0, reg.STRICT_RATIO) as m:
                out["one_map_ms_per_iteration"] = round(best_ms(lambda: m.register(sc, frames, s["poses"], **opts), a.repeat) / a.iterations, 4)
            with sc.submaps(s["poses_gt"], 1, 1.0, reg.STRICT_RATIO) as sm:
                other = (frames + 1) % a.jobs                                # every frame against its neighbour's submap
                out["submaps_ms_per_iteration"] = round(best_ms(lambda: sm.register(sc, frames, other, s["poses"], **opts), a.repeat) / a.iterations, 4)
                out["submaps"] = sm.n_submaps
        out.update(jobs=a.jobs, points_per_job=a.points, iterations=a.iterations)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
