"""Pair-selection timings: lvba_covis_pairs on synthetic depth images (a plane before every camera, with holes, uploaded with
lvba_depth_upload) and cameras on a loop, beside the numpy restatement and beside what the selection saves the matcher.

    python tools/covis_bench.py [--images 256 1024 2048] [--repeat 3] [--oracle-images 256] [--match-images 256] [--match-keypoints 1024]

Prints one JSON line.  Times are the host clock around calls that end in a device synchronise and include the upload of the poses
and the copy of the pairs to the host (best of --repeat, after a warm-up call); the depth images are resident before the clock
starts; every timed call has room for all its pairs, so it is one call.  "cap8_ms" adds max_per_image = 8, the only option that runs the select kernel.
"oracle_ms" is tests/covis_oracle.py on the first --oracle-images images: single-threaded numpy, a restatement of the rule and not
a tuned CPU code.  "match": depth-guided matching (match.Matcher, guided = 2) of --match-keypoints random descriptors per image
over all pairs and over the selected pairs of the first --match-images images -- the number that says whether the selection
pays.  The kernels' own times come from a run under `rocprofv3 --kernel-trace --stats` with --no-oracle --no-match.  Needs a HIP
device."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best_ms(fn, repeat):
    fn()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(min(ms), 3)


def scene(M, W, H, seed):
    """cameras on a circle of 0.5 m per image, looking along the tangent; depth: a plane 6 .. 10 m before each, a fifth of it holes"""
    import match_cases as mc
    synth = importlib.import_module("global-lvba_amd.synth")
    rng = np.random.default_rng(seed)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    a = 2.0 * np.pi * np.arange(M) / M
    radius = 0.5 * M / (2.0 * np.pi)
    C = np.stack([radius * np.cos(a), np.zeros(M), radius * np.sin(a)], 1)
    Rcw = np.stack([mc._rot(0.0, y, 0.0).T for y in np.arctan2(-np.sin(a), np.cos(a))])
    tcw = -np.einsum("nij,nj->ni", Rcw, C)
    base = np.ones((H, W), np.float32)
    for _ in range(40):
        x, y = int(rng.integers(0, W - 64)), int(rng.integers(0, H - 64))
        base[y:y + int(rng.integers(8, 64)), x:x + int(rng.integers(8, 64))] = 0
    depth = np.ascontiguousarray(np.broadcast_to(base, (M, H, W)))
    depth *= (6.0 + 4.0 * rng.uniform(size=M)).astype(np.float32)[:, None, None]
    return depth, intr, Rcw, tcw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[256, 1024, 2048])
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--oracle-images", type=int, default=256)
    ap.add_argument("--match-images", type=int, default=256)
    ap.add_argument("--match-keypoints", type=int, default=1024)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--no-match", action="store_true")
    args = ap.parse_args()
    L = importlib.import_module("global-lvba_amd._lib")
    if L.load().lvba_device_count() < 1:
        raise SystemExit("covis_bench needs a HIP device")
    CV = importlib.import_module("global-lvba_amd.covis")
    V = importlib.import_module("global-lvba_amd.visual")
    out = dict(width=args.width, height=args.height, grid=[16, 12], sizes=[])
    for M in args.images:
        depth, intr, Rcw, tcw = scene(M, args.width, args.height, 7)
        row = dict(images=M, all_pairs=M * (M - 1) // 2)
        with V.DepthImages.upload(depth) as d:
            for name, kw in (("on", dict()), ("off", dict(occlusion=0)), ("cap8", dict(max_per_image=8))):
                cap = row[name + "_selected"] = len(CV.select_pairs(d, Rcw, tcw, intr, **kw)[0])      # one call, with room for all
                row[name + "_ms"] = best_ms(lambda: CV.select_pairs(d, Rcw, tcw, intr, capacity=cap, **kw), args.repeat)
            row["samples_ms"] = best_ms(lambda: CV.samples(d, Rcw, tcw, intr), args.repeat)
            if not args.no_oracle and M == args.oracle_images:
                import covis_oracle as co
                t0 = time.perf_counter()
                want = co.select_pairs(depth, intr, Rcw, tcw)
                row["oracle_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                row["oracle_equal"] = bool(np.array_equal(want[0], CV.select_pairs(d, Rcw, tcw, intr)[0]))
            if not args.no_match and M == args.match_images:
                import match_cases as mc
                Mt = importlib.import_module("global-lvba_amd.match")
                rng = np.random.default_rng(11)
                n = args.match_keypoints
                descs = list(mc.sift_like(rng, M * n).reshape(M, n, 128))
                kps = [np.stack([rng.uniform(2, args.width - 3, n), rng.uniform(2, args.height - 3, n)], 1).astype(np.float32) for _ in range(M)]
                every = [(i, j) for i in range(M) for j in range(i + 1, M)]
                chosen = CV.select_pairs(d, Rcw, tcw, intr)[0]
                with Mt.Matcher(descs) as m:
                    m.set_geometry(kps, intr, Rcw, tcw)
                    m.set_depth(d)
                    row["match"] = dict(keypoints=n, all_pairs_ms=best_ms(lambda: m.match_pairs_csr(every, guided=2), 1),
                                        selected_pairs=len(chosen),
                                        selected_ms=best_ms(lambda: m.match_pairs_csr(chosen, guided=2), args.repeat))
        out["sizes"].append(row)
        del depth
    print(json.dumps(out))


if __name__ == "__main__":
    main()
