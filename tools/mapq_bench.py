"""Times the map-quality metrics (lvba_mapq_scans) on 64 frames x 100 k points of synth.make_scans, radius 0.3 m, query strides 1
and 8.  Prints one JSON line per stride: ms per stage (world points, sort + cell table, reduction, download), points/s,
queries/s and neighbour visits/s (candidates tested, = sum of the 27-cell populations over the queries, counted on the host
from the cell histogram) against the fp64 vector rate of the device; then the brute-force restatement (tests/mapq_oracle.py)
on the largest prefix of the cloud it finishes in <= 30 s, with the cores it used.

Each GPU step is a child process under its own `timeout -k 10`; a step that fails ends the run.

    usage: mapq_bench.py [frames] [pts] [--no-oracle]          (child: mapq_bench.py --step STRIDE frames pts)"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RADIUS, MIN_NB = 0.3, 8
FP64_VECTOR_FLOPS = 78.6e12      # MI355X peak fp64 vector rate
FLOPS_PER_VISIT = 9              # 3 subtractions, 3 products, 2 additions, 1 comparison; + 18 for a candidate inside the radius


def scene(frames, ppf):
    synth = importlib.import_module("global-lvba_amd.synth")
    s = synth.make_scans(frames, ppf)
    return s["clouds"], np.asarray(s["poses_gt"], np.float64).reshape(-1, 12)


def visits(world, stride):
    """Candidates the reduction tests: for every query, the points of the 27 cells around it (edge = radius (1 + 2^-20))."""
    w = world[np.isfinite(world).all(1)].astype(np.float64)
    c = np.floor(w / (RADIUS * (1 + 2.0 ** -20))).astype(np.int64)
    c -= c.min(0)
    dim = c.max(0) + 3
    grid = np.zeros(tuple(dim), np.int64)
    np.add.at(grid, (c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1), 1)
    box = sum(np.roll(grid, (a, b, d), (0, 1, 2)) for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1))
    q = c[::stride]                                              # (the scene has no non-finite point)
    return int(box[q[:, 0] + 1, q[:, 1] + 1, q[:, 2] + 1].sum())


def step(stride, frames, ppf):
    pkg = importlib.import_module("global-lvba_amd")
    mq = importlib.import_module("global-lvba_amd.mapq")
    clouds, poses = scene(frames, ppf)
    with pkg.Scans(clouds) as scans:
        best = None
        for rep in range(3):                                     # the first run warms the pool and the kernels up
            t0 = time.perf_counter()
            r = mq.map_quality_scans(scans, poses, radius=RADIUS, min_neighbors=MIN_NB, query_stride=stride)
            wall = time.perf_counter() - t0
            if rep and (best is None or r["ms"]["reduce"] < best[0]["ms"]["reduce"]):
                best = (r, wall)
    r, wall = best
    mo = importlib.import_module("mapq_oracle")
    nv = visits(mo.world_points([np.asarray(c, np.float32)[:, :3] for c in clouds], poses), stride)
    red_s = r["ms"]["reduce"] * 1e-3
    inside = r["mean_neighbors"] * r["n_queries"]
    flops = FLOPS_PER_VISIT * nv + 18 * inside
    print(json.dumps(dict(stride=stride, n_points=r["n_points"], n_queries=r["n_queries"], n_valid=r["n_valid"], mme=r["mme"], mpv=r["mpv"],
                          mean_neighbors=r["mean_neighbors"], ms=r["ms"], wall_ms=1e3 * wall, points_per_s=r["n_points"] / wall,
                          queries_per_s=r["n_queries"] / red_s, visits=nv, visits_per_s=nv / red_s,
                          fp64_vector_share=flops / red_s / FP64_VECTOR_FLOPS,
                          record_bytes_per_s_if_unshared=16.0 * nv / red_s)))


def oracle_prefix(frames, ppf):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    mo = importlib.import_module("mapq_oracle")
    clouds, poses = scene(frames, ppf)
    world = mo.world_points([np.asarray(c, np.float32)[:, :3] for c in clouds], poses)
    n, last = 2000, None
    while n <= len(world):
        t0 = time.perf_counter()
        mo.metrics(world[:n], RADIUS, MIN_NB)
        dt = time.perf_counter() - t0
        if dt > 30.0:
            break
        last = (n, dt)
        if dt * 4 > 30.0:                                        # O(n^2): the next doubling would not finish
            break
        n *= 2
    print(json.dumps(dict(oracle_prefix_points=last[0], oracle_s=last[1], oracle_points_per_s=last[0] / last[1], cores_used=1,
                          cores_present=os.cpu_count())))


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--step" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        step(int(argv[0]), int(argv[1]), int(argv[2]))
        sys.exit(0)
    frames = int(argv[0]) if len(argv) > 0 else 64
    ppf = int(argv[1]) if len(argv) > 1 else 100000
    for stride in (1, 8):
        rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", str(stride), str(frames), str(ppf)])
        if rc != 0:
            sys.exit(rc)
    if "--no-oracle" not in sys.argv:
        oracle_prefix(frames, ppf)
