#!/usr/bin/env python3
"""Time the SIFT extractor (features.extract): ms per image and per stage for 64 images of 1280 x 1024 and of
640 x 512, with first_octave = -1 and 0, next to the bytes per image that the pixel passes are modelled to move.  A side tool: no
test runs it.

    python tools/sift_bench.py [--images 64] [--repeats 3] [--out sift_bench.json]

The images are seeded plane-wave textures (thousands of key points each).  The stage times are the library's own, by the host's
clock at points where the stream is drained (features.last_profile); the first call of every shape is a warm-up and not counted."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def texture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.zeros((h, w), np.float32)
    for _ in range(24):
        k = rng.normal(size=2)
        k *= (2 * np.pi / rng.uniform(6.0, 60.0)) / np.linalg.norm(k)
        a += np.float32(rng.uniform(0.5, 1.0)) * np.sin(np.float32(k[0]) * xx + np.float32(k[1]) * yy + np.float32(rng.uniform(0, 6.28)))
    g = np.clip(np.rint(128.0 + 22.0 * a), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], 2))


def modelled_bytes(w, h, channels, first_octave, S=3):
    """Bytes per image that the pixel passes read and write, from the shapes alone (re-reads that a cache serves are not counted:
    the 3 x 3 neighbourhoods of the detection pass, the halos of the blur tiles)."""
    ow, oh = (2 * w, 2 * h) if first_octave < 0 else (w, h)
    total = w * h * channels + 4 * ow * oh                       # the base image: bytes in, floats out
    first = True
    while True:
        npx = ow * oh
        blurs = (S + 3) if first else (S + 2)                     # the base blur belongs to the first octave
        total += blurs * 16 * npx                                 # rows: 4 in + 4 out; columns: 4 in + 4 out
        total += 4 * npx * ((S + 3) + (S + 2) + S)                # detection: the Gaussian levels in, DoG levels and flags out
        total += 4 * npx * S * 4                                  # the scan (flags in, places out) and the gather (both in)
        ow, oh, first = ow // 2, oh // 2, False
        if min(ow, oh) < 8:
            return total
        total += 4 * ow * oh * 3                                  # level S at every second pixel, and its copy into place


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ft = importlib.import_module("global-lvba_amd.features")
    L = importlib.import_module("global-lvba_amd._lib")
    if L.load().lvba_device_count() < 1:
        raise SystemExit("sift_bench needs a HIP device: a time taken anywhere else says nothing")
    rows = []
    for w, h in ((1280, 1024), (640, 512)):
        base = [texture(w, h, s) for s in range(8)]
        imgs = [base[k % 8] if k < 8 else np.ascontiguousarray(np.roll(base[k % 8], 17 * k, axis=1)) for k in range(args.images)]
        for fo in (-1, 0):
            ft.extract(imgs[:min(8, len(imgs))], first_octave=fo)                   # warm-up: code objects, pools
            ft.extract(imgs, first_octave=fo)
            best = None
            for _ in range(args.repeats):
                t = time.perf_counter()
                kp, ds, counts = ft.extract(imgs, first_octave=fo)
                wall = (time.perf_counter() - t) * 1e3
                prof = ft.last_profile()
                if best is None or wall < best["wall_ms"]:
                    best = dict(wall_ms=wall, **{f"{k}_ms": v for k, v in prof.items()})
            n = len(imgs)
            row = dict(width=w, height=h, first_octave=fo, images=n, features_per_image=float(np.mean([len(k) for k in kp])),
                       found_per_image=float(np.mean(counts)), modelled_MB_per_image=modelled_bytes(w, h, 3, fo) / 1e6,
                       **{k.replace("_ms", "_ms_per_image"): v / n for k, v in best.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
