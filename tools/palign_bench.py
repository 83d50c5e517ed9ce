"""Times one linearisation pass of the photometric camera alignment (lvba_palign_*, csrc/palign.hip): 10^6 and 10^7
map points against 64 to 1 024 images of 1 280 x 1 024 with depth images, at the default options.  Beside it, on the same inputs in
the same run: the sample pass of the colour fusion (lvba_photo_*, the yardstick: the same projection, occlusion test and texel
gathers, without the gradient, the Jacobian and the 31 sums), and both passes with the points moved out of every view
("projection_only"), where no pair survives the projection.  No test runs this.  The numbers go into DESIGN.md §10q and a JSON file:

    python tools/palign_bench.py --out profiles/palign_bench.json [--points 1000000 10000000] [--images 64 256 1024]

The scene is tools/photo_bench.py's: a box room, points uniform on its walls, 8 rendered views, image k = view k % 8.  The
reference colours are the planted colours of the points.  Times are the library's own device events around the kernels.  Every
shape is warmed up once; then `reps` handles are timed and the mean, the smallest and the largest are reported."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

try:
    import torch  # noqa: F401                                        # first: its HIP runtime must be the one in the process
except Exception:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import photo_bench as pb  # noqa: E402


def planted_ref16(P):
    P = P.astype(np.float64)
    col = 127.5 + 100.0 * np.stack([np.sin(0.8 * (P[:, 0] + 0.5 * P[:, 1])), np.cos(0.8 * (P[:, 2] + 0.3 * P[:, 0])),
                                    np.sin(0.8 * (1.5 * P[:, 1] + 0.7 * P[:, 2]) + 1.0)], 1)
    return np.floor(col * 256.0 + 0.5).astype(np.uint16)


def stats(v):
    return dict(mean=sum(v) / len(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--images", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--target-proj", type=float, default=1e10, help="projections the timed passes of a shape add up to")
    ap.add_argument("--max-reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    PA = importlib.import_module("global-lvba_amd.palign")
    PH = importlib.import_module("global-lvba_amd.photo")
    V = importlib.import_module("global-lvba_amd.visual")
    if importlib.import_module("global-lvba_amd._lib").load().lvba_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    rng = np.random.default_rng(3)
    Rv, tv, dv, iv = pb.views()
    pts_all = pb.wall_points(max(a.points), rng)
    ref_all = planted_ref16(pts_all)
    valid_all = np.ones(len(pts_all), np.uint8)
    rows = []
    for M in a.images:
        pick = np.arange(M) % pb.N_VIEWS
        Rcw, tcw = np.ascontiguousarray(Rv[pick]), np.ascontiguousarray(tv[pick])
        images, depth_host = np.ascontiguousarray(iv[pick]), np.ascontiguousarray(dv[pick])
        with V.DepthImages.upload(depth_host) as depth:
            del depth_host
            for n, kind in [(n, kind) for n in a.points for kind in ("scene", "projection_only")]:
                pts = pts_all[:n] if kind == "scene" else pts_all[:n] + np.array([0, 0, 1000.0], np.float32)
                pairs = float(n) * M
                reps = int(min(a.max_reps, max(1, math.ceil(a.target_proj / pairs))))
                lin_ms, step_ms, photo_ms = [], [], []
                for r in range(reps + 1):                             # run 0 warms the shape up
                    with PA.PhotoAligner(pts, ref_all[:n], valid_all[:n], M, pb.W, pb.H, pb.INTR, depth=depth) as al:
                        res = al.linearize(0, Rcw, tcw, images)
                        p = al.profile()
                    with PH.PhotoMap(pts, M, pb.INTR, pb.W, pb.H, depth=depth) as pm:
                        pm.add_images(0, Rcw, tcw, images)
                        s = pm.finish()["summary"]
                    if r:
                        lin_ms.append(p["linearize"]); step_ms.append(p["step"]); photo_ms.append(s["ms"][1])
                samples = int(res["n_samples"].sum())
                assert samples == s["n_samples"], (samples, s["n_samples"])   # every point is valid: the fusion samples the same pairs
                lin, pho = stats(lin_ms), stats(photo_ms)
                row = dict(kind=kind, n_points=n, n_images=M, width=pb.W, height=pb.H, projections=pairs, samples=samples, reps=reps,
                           linearize_ms=lin, step_ms=stats(step_ms), photo_sample_ms=pho, ratio_to_photo=lin["mean"] / pho["mean"],
                           proj_per_s=pairs / (lin["mean"] * 1e-3), samples_per_s=samples / (lin["mean"] * 1e-3),
                           photo_proj_per_s=pairs / (pho["mean"] * 1e-3), image_bytes=int(images.nbytes))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(dict(tool="tools/palign_bench.py", options="defaults", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
