"""Times the sums pass of the exposure estimation (lvba_expo_sums, csrc/expo.hip) on the shapes of
tools/photo_bench.py: 10^6 and 10^7 map points against 64 to 1 024 images of 1 280 x 1 024 with depth images, at the default
options.  Beside it, in the same run and alternating with it repetition by repetition, on the same inputs: the fusion's sample
pass in its plain and in its gains instantiation, and one linearisation of the photometric alignment (lvba_palign_linearize).
No test runs this.  The numbers go into DESIGN.md §10r and a JSON file:

    python tools/expo_bench.py --out profiles/expo_bench.json [--points 1000000 10000000] [--images 64 256 1024]

The scene is photo_bench's; image k carries a gain of 0.8 .. 1.25 applied to its bytes, and the gains the passes are given undo
it.  The reference colours are those of a plain fusion of the same images.  Times are the library's own device events around
each pass.  Every shape is warmed up once (every pass once); then `reps` rounds are timed, each round running the four passes
one after the other, enough rounds that a pass's timed window adds up to about 2 x 10^10 projections, and the mean, the smallest
and the largest are reported."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

try:
    import torch                                                      # first: its HIP runtime must be the one in the process
except Exception:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import photo_bench as pb                                              # noqa: E402  (the scene)

PASSES = ("sample_plain", "sample_gains", "expo_sums", "palign_linearize")


def stats(v):
    return dict(mean=sum(v) / len(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--images", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--target-proj", type=float, default=2e10, help="projections the timed passes of a shape add up to, per pass")
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    PH = importlib.import_module("global-lvba_amd.photo")
    PA = importlib.import_module("global-lvba_amd.palign")
    EX = importlib.import_module("global-lvba_amd.expo")
    V = importlib.import_module("global-lvba_amd.visual")
    if importlib.import_module("global-lvba_amd._lib").load().lvba_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    W, H, INTR = pb.W, pb.H, pb.INTR
    rng = np.random.default_rng(3)
    Rv, tv, dv, iv = pb.views()
    pts_all = pb.wall_points(max(a.points), rng)
    rows = []
    for M in a.images:
        pick = np.arange(M) % pb.N_VIEWS
        planted = np.exp(rng.uniform(np.log(0.8), np.log(1.25), M))
        Rcw, tcw = np.ascontiguousarray(Rv[pick]), np.ascontiguousarray(tv[pick])
        images = np.empty((M, H, W, 3), np.uint8)
        for k in range(M):
            images[k] = np.clip(np.floor(planted[k] * iv[pick[k]].astype(np.float32) + 0.5), 0, 255)
        gains = EX.identity_gains(M)
        gains[:, :, 0] = np.floor(65536.0 / planted + 0.5).astype(np.int64)[:, None]
        with V.DepthImages.upload(np.ascontiguousarray(dv[pick])) as depth:
            for n in a.points:
                pts = pts_all[:n]
                pairs = float(n) * M
                reps = int(min(a.max_reps, max(1, math.ceil(a.target_proj / pairs))))
                with PH.PhotoMap(pts, M, INTR, W, H, depth=depth) as pm:
                    pm.add_images(0, Rcw, tcw, images, gains=gains)
                    nv, s1, _ = pm.sums()
                ref16, valid = PA.reference_from_sums(nv, s1)
                t = {k: [] for k in PASSES}
                with EX.ExposureEstimator(pts, ref16, valid, M, W, H, INTR, depth=depth) as est, \
                        PA.PhotoAligner(pts, ref16, valid, M, W, H, INTR, depth=depth) as pa:
                    before_e, before_p = 0.0, 0.0
                    for r in range(reps + 1):                         # round 0 warms every pass up
                        for g in (None, gains):
                            with PH.PhotoMap(pts, M, INTR, W, H, depth=depth) as pm:
                                pm.add_images(0, Rcw, tcw, images, **({} if g is None else dict(gains=g)))
                                ms = pm.finish()["summary"]["ms"][1]
                            if r:
                                t["sample_plain" if g is None else "sample_gains"].append(ms)
                        sums = est.sums(0, Rcw, tcw, images, gains=gains)
                        now = est.profile()["sums"]
                        if r:
                            t["expo_sums"].append(now - before_e)
                        before_e = now
                        pa.linearize(0, Rcw, tcw, images)
                        now = pa.profile()["linearize"]
                        if r:
                            t["palign_linearize"].append(now - before_p)
                        before_p = now
                row = dict(n_points=n, n_images=M, width=W, height=H, projections=pairs, reps=reps, n_valid=int(valid.sum()),
                           located=int(sums[:, 18].sum()), used_terms=int(sums[:, 0:18:6].sum()), refused_terms=int(sums[:, 19].sum()),
                           **{k + "_ms": stats(v) for k, v in t.items()},
                           expo_sums_proj_per_s=pairs / (stats(t["expo_sums"])["mean"] * 1e-3),
                           expo_sums_over_sample_plain=stats(t["expo_sums"])["mean"] / stats(t["sample_plain"])["mean"],
                           expo_sums_over_palign_linearize=stats(t["expo_sums"])["mean"] / stats(t["palign_linearize"])["mean"],
                           sample_gains_over_plain=stats(t["sample_gains"])["mean"] / stats(t["sample_plain"])["mean"])
                rows.append(row)
                print(json.dumps(row), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(dict(tool="tools/expo_bench.py", options="defaults", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
