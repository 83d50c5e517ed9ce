"""Times the three passes of lvba_dynamic_labels (range images, dilation, votes) on synthetic sequences: 500 and 2 000 frames of
5 000 and 20 000 points, with window 20 and with every frame voting, at the default options; and, beside them, the time of the
numpy restatement (tests/dynamic_oracle.py) for a slice of the same projections on the host, as the CPU baseline.  No test runs
this.  The numbers go into DESIGN.md §10m and a JSON file:

    python tools/dynamic_bench.py --out profiles/dynamic_bench.json [--frames 500 2000] [--points 5000 20000] [--max-gproj 100]

A sequence: a box room of 60 x 40 x 6 m, the sensor on a loop through it (one frame every 0.25 m), rays uniform in azimuth and
in elevation over +-60 degrees, every ray ends on the room.  Every configuration runs twice; the second run is reported."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROOM = np.array([30.0, 20.0, 3.0], np.float32)   # half extents


def sequence(n_frames, n_points, seed=7):
    rng = np.random.default_rng(seed)
    s = 0.25 * np.arange(n_frames) / 18.0                                # arc length over the loop's mean radius
    pos = np.stack([20.0 * np.cos(s), 12.0 * np.sin(s), 0.5 * np.sin(3.0 * s)], 1)
    yaw = s + np.pi / 2
    clouds, poses = [], []
    for f in range(n_frames):
        az = rng.uniform(-np.pi, np.pi, n_points).astype(np.float32)
        el = rng.uniform(-np.pi / 3, np.pi / 3, n_points).astype(np.float32)
        d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
        c, sn = np.float32(np.cos(yaw[f])), np.float32(np.sin(yaw[f]))
        dw = np.stack([c * d[:, 0] - sn * d[:, 1], sn * d[:, 0] + c * d[:, 1], d[:, 2]], 1)
        p = pos[f].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(dw > 0, (ROOM - p) / dw, np.where(dw < 0, (-ROOM - p) / dw, np.inf)).min(1)
        clouds.append(np.ascontiguousarray(d * t[:, None], np.float32))
        poses.append([np.cos(yaw[f]), -np.sin(yaw[f]), 0, np.sin(yaw[f]), np.cos(yaw[f]), 0, 0, 0, 1, *pos[f]])
    return clouds, np.array(poses, np.float64)


def host_slice(clouds, poses, window, n_points=2000, n_voters=8):
    """the numpy oracle on the first n_points points of the middle frame against n_voters frames of its window: seconds for
    their images and for the projections with their votes, and the number of projections"""
    do = importlib.import_module("dynamic_oracle")
    f = len(clouds) // 2
    voters = [g for g in range(f - n_voters // 2, f + n_voters // 2 + 1) if g != f and 0 <= g < len(clouds)][:n_voters]
    o = do.options(window=window)
    t0 = time.perf_counter()
    M = {g: do.dilate(do.range_image(clouds[g], **o)[0], o["halo"]) for g in voters}
    t1 = time.perf_counter()
    w = do.world_points(clouds[f][:n_points], poses[f])
    votes = 0
    for g in voters:
        q = do.cells(do.to_body(w, poses[g]), **o)
        has = q["cell"] >= 0
        m = np.where(has, M[g].reshape(-1)[np.where(has, q["cell"], 0)], np.inf).astype(np.float64)
        tol = o["abs_tol"] + o["rel_tol"] * q["r"]
        votes += int((has & np.isfinite(m) & (m >= q["r"] - tol)).sum())
    t2 = time.perf_counter()
    return dict(images_s=t1 - t0, votes_s=t2 - t1, projections=len(w) * len(voters), images=len(voters), votes=votes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--points", type=int, nargs="+", default=[5000, 20000])
    ap.add_argument("--windows", type=int, nargs="+", default=[20, 0])
    ap.add_argument("--max-gproj", type=float, default=0.0, help="skip configurations with more than this many 1e9 projections (0: none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("global-lvba_amd")
    dyn = importlib.import_module("global-lvba_amd.dynamic")
    rows = []
    for n_points in a.points:
        for n_frames in a.frames:
            clouds, poses = sequence(n_frames, n_points)
            with pkg.Scans(clouds) as scans:
                for window in a.windows:
                    voters = np.minimum(np.arange(n_frames) + window, n_frames - 1) - np.maximum(np.arange(n_frames) - window, 0) \
                        if window > 0 else np.full(n_frames, n_frames - 1)
                    proj = float(voters.sum()) * n_points
                    row = dict(n_frames=n_frames, n_points=n_points, window=window, projections=proj)
                    if a.max_gproj and proj > a.max_gproj * 1e9:
                        row["skipped"] = f"more than {a.max_gproj:g}e9 projections"
                    else:
                        for _ in range(2):
                            r = dyn.dynamic_labels(scans, poses, per_point=False, window=window)
                        row.update(ms=r["ms"], n_judged=r["n_judged"], n_dynamic=r["n_dynamic"],
                                   gproj_per_s=proj / max(r["ms"]["votes"], 1e-9) / 1e6)
                        row["host"] = host_slice(clouds, poses, window)
                        row["host_gproj_per_s"] = row["host"]["projections"] / row["host"]["votes_s"] / 1e9
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    if a.out:
                        with open(a.out, "w") as f:
                            json.dump(dict(tool="tools/dynamic_bench.py", options="defaults (240 x 720, halo 1)", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
