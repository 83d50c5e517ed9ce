"""Times the sample pass of the multi-view colour fusion (lvba_photo_*, csrc/photo.hip): 10^6 and 10^7 map points
against 64 to 1 024 images of 1 280 x 1 024 with depth images, at the default options.  Beside it, in the same run: the time of a
device-to-device copy of the same image bytes (what merely touching the images costs), and the rate of the numpy restatement
(tests/photo_oracle.py) at a size it can finish, as the CPU baseline.  No test runs this.  The numbers go into DESIGN.md §10p and
a JSON file:

    python tools/photo_bench.py --out profiles/photo_bench.json [--points 1000000 10000000] [--images 64 256 1024]

The scene: a box room of 30 x 20 x 6 m, points uniform on its walls, N_VIEWS cameras on a loop through it looking along the
tangent; image k is view k % N_VIEWS (its rendered colours and its analytic depth image), so that the host renders N_VIEWS images
however many the device samples.  Times are device events (the library's own, around the sample kernel and around the upload;
torch's around the copy).  Every shape is warmed up once with a handle of its own; then `reps` handles are timed,
enough of them that the timed sample passes add up to about 2 x 10^10 projections, and the mean, the smallest and the largest
are reported.  Every shape is timed twice: on the scene, and with the points moved out of every view ("projection_only"), where no
pair survives the projection and the pass does its arithmetic and no gather."""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

try:
    import torch                                                      # first: its HIP runtime must be the one in the process
except Exception:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HALF = np.array([15.0, 10.0, 3.0])                                    # the room's half extents
W, H = 1280, 1024
INTR = np.array([646.78472, 646.65775, 313.456795 * 2, 261.399612 * 2, -0.076160, 0.123001, -0.00113, 0.000251])
N_VIEWS = 8
VOTE_PASS_RATE = 1.0e11                                               # projections per second of dyn_vote_kernel


def wall_points(n, rng):
    """float32 [n, 3] uniform on the six walls, by area"""
    area = np.array([HALF[1] * HALF[2], HALF[0] * HALF[2], HALF[0] * HALF[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    p = rng.uniform(-1, 1, (n, 3)) * HALF
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * HALF[axis]
    return np.ascontiguousarray(p, np.float32)


def cast(origin, dirs):
    """the parameter of the wall along origin + s dirs (the origin is inside the room)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dirs > 0, (HALF - origin) / dirs, np.where(dirs < 0, (-HALF - origin) / dirs, np.inf)).min(1)


def views():
    """(Rcw [N_VIEWS, 3, 3], tcw, depth float32 [N_VIEWS, H, W], images uint8 [N_VIEWS, H, W, 3])"""
    co = importlib.import_module("covis_oracle")
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y, ok = co.undistort(INTR, u.ravel(), v.ravel())
    assert ok.all()
    rays = np.stack([x, y, np.ones_like(x)], 1)
    R, t, depth, images = [], [], [], []
    for k in range(N_VIEWS):
        a = 2 * np.pi * k / N_VIEWS
        C = np.array([9.0 * np.cos(a), 5.0 * np.sin(a), 0.3 * np.sin(3 * a)])
        fwd = np.array([-9.0 * np.sin(a), 5.0 * np.cos(a), 0.0])
        fwd /= np.linalg.norm(fwd)
        down = np.array([0.0, 0.0, -1.0])
        Rk = np.stack([np.cross(down, fwd), down, fwd])               # rows: the camera's x, y, z axes in the world
        dirs = rays @ Rk
        s = cast(C, dirs)
        P = C + s[:, None] * dirs
        col = 127.5 + 100.0 * np.stack([np.sin(0.8 * (P[:, 0] + 0.5 * P[:, 1])), np.cos(0.8 * (P[:, 2] + 0.3 * P[:, 0])),
                                        np.sin(0.8 * (1.5 * P[:, 1] + 0.7 * P[:, 2]) + 1.0)], 1)
        R.append(Rk); t.append(-Rk @ C)
        depth.append(s.astype(np.float32).reshape(H, W))
        images.append(np.floor(col + 0.5).astype(np.uint8).reshape(H, W, 3))
    return np.array(R), np.array(t), np.array(depth), np.array(images)


def device_copy_ms(n_bytes, reps=5):
    """device events around a device-to-device copy of n_bytes (in pieces of at most 2 GiB), after one warm-up: the best of reps"""
    piece = min(n_bytes, 1 << 31)
    src = torch.empty(piece, dtype=torch.uint8, device="cuda").fill_(7)
    dst = torch.empty_like(src)
    best = math.inf
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        done = 0
        while done < n_bytes:
            m = min(piece, n_bytes - done)
            dst[:m].copy_(src[:m])
            done += m
        e1.record()
        torch.cuda.synchronize()
        if r:
            best = min(best, e0.elapsed_time(e1))
    return best


def host_rate(points, Rcw, tcw, depth, images, n_points=20000, n_images=4):
    po = importlib.import_module("photo_oracle")
    t0 = time.perf_counter()
    nv = po.sums(points[:n_points], images[:n_images], depth[:n_images], INTR, Rcw[:n_images], tcw[:n_images])[0]
    dt = time.perf_counter() - t0
    return dict(points=n_points, images=n_images, seconds=dt, proj_per_s=n_points * n_images / dt, samples_per_s=float(nv.sum()) / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--images", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--target-proj", type=float, default=2e10, help="projections the timed sample passes of a shape add up to")
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    PH = importlib.import_module("global-lvba_amd.photo")
    V = importlib.import_module("global-lvba_amd.visual")
    if importlib.import_module("global-lvba_amd._lib").load().lvba_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    rng = np.random.default_rng(3)
    Rv, tv, dv, iv = views()
    pts_all = wall_points(max(a.points), rng)
    rows = [dict(host=host_rate(pts_all, Rv, tv, dv, iv))]
    print(json.dumps(rows[0]), flush=True)
    for M in a.images:
        pick = np.arange(M) % N_VIEWS
        Rcw, tcw = np.ascontiguousarray(Rv[pick]), np.ascontiguousarray(tv[pick])
        images, depth_host = np.ascontiguousarray(iv[pick]), np.ascontiguousarray(dv[pick])
        copy_ms = device_copy_ms(images.nbytes) if torch is not None else None
        with V.DepthImages.upload(depth_host) as depth:
            del depth_host
            for n, kind in [(n, kind) for n in a.points for kind in ("scene", "projection_only")]:
                # projection_only: the same points 1 000 m away along z, where every (point, image) pair ends at BEHIND or OUTSIDE
                # after the projection and nothing is gathered -- what the arithmetic alone costs
                pts = pts_all[:n] if kind == "scene" else pts_all[:n] + np.array([0, 0, 1000.0], np.float32)
                pairs = float(n) * M
                reps = int(min(a.max_reps, max(1, math.ceil(a.target_proj / pairs))))
                runs = []
                for r in range(reps + 1):                             # run 0 warms the shape up
                    with PH.PhotoMap(pts, M, INTR, W, H, depth=depth) as pm:
                        t0 = time.perf_counter()
                        pm.add_images(0, Rcw, tcw, images)
                        call_ms = 1e3 * (time.perf_counter() - t0)
                        s = pm.finish()["summary"]
                    if r:
                        runs.append(dict(call_ms=call_ms, upload_ms=s["ms"][0], sample_ms=s["ms"][1], finish_ms=s["ms"][2],
                                         download_ms=s["ms"][3]))
                sample = [x["sample_ms"] for x in runs]
                mean = sum(sample) / len(sample)
                row = dict(kind=kind, n_points=n, n_images=M, width=W, height=H, projections=pairs, samples=s["n_samples"], n_seen=s["n_seen"],
                           n_valid=s["n_valid"], mean_sigma=s["mean_sigma"], mean_views=s["mean_views"], reps=reps,
                           sample_ms=dict(mean=mean, min=min(sample), max=max(sample)), timed_window_ms=sum(sample),
                           call_ms=sum(x["call_ms"] for x in runs) / len(runs), upload_ms=sum(x["upload_ms"] for x in runs) / len(runs),
                           finish_ms=sum(x["finish_ms"] for x in runs) / len(runs),
                           download_ms=sum(x["download_ms"] for x in runs) / len(runs),
                           proj_per_s=pairs / (mean * 1e-3), samples_per_s=s["n_samples"] / (mean * 1e-3),
                           of_vote_pass=pairs / (mean * 1e-3) / VOTE_PASS_RATE, image_bytes=int(images.nbytes),
                           device_copy_ms=copy_ms if copy_ms is not None else "not measured")
                rows.append(row)
                print(json.dumps(row), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(dict(tool="tools/photo_bench.py", options="defaults", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
