"""Descriptor-matching timings: lvba_match_pairs on synthetic SIFT-like descriptors, few large pairs against many small ones,
unguided, guided by the epipolar line and guided by LiDAR depth, beside the numpy restatement on a pair of the same size.

    python tools/match_bench.py [--sizes 2048 8192 32768] [--small 256] [--small-pairs 2000] [--repeat 3] [--oracle-size 2048]

Prints one JSON line.  Times are the host clock around calls that end in a device synchronise and include the copy of the matches
to the host (best of --repeat, after a warm-up call).  "tmacs" counts n_a n_b 128 integer multiply-adds per ordered scan, two
scans per pair when mutual.  "oracle_ms" is tests/match_oracle.py on one pair: a single-threaded numpy int64 matrix product and
its arg-max, a restatement of the rule and not a tuned CPU matcher.  The depth images of the depth-guided column are synthetic: a
plane 8 m before every camera, uploaded with lvba_depth_upload; "set_depth_ms" is the lifting of all keypoints through them
(lvba_match_set_depth, once per pose set), which the column's own time does not include.  Needs a HIP device."""
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


def images(n_images, n, seed):
    """n_images images of n descriptors: two thirds re-observe a common pool, the rest are distractors; keypoints and poses of a
    camera moving sideways past points 6 to 11 m away"""
    import match_cases as mc
    synth = importlib.import_module("global-lvba_amd.synth")
    rng = np.random.default_rng(seed)
    shared = (2 * n) // 3
    pool = mc.sift_like(rng, shared)
    intr = np.asarray(synth.REF_INTRINSICS, np.float64)
    fx, fy, cx, cy = intr[:4]
    X = np.stack([rng.uniform(-3, 3, shared), rng.uniform(-2, 2, shared), rng.uniform(6, 11, shared)], 1)
    W, H = synth.REF_IMAGE_WH
    descs, kps = [], []
    for v in range(n_images):
        p = rng.permutation(n)
        d = np.vstack([mc.noisy(rng, pool, 12), mc.sift_like(rng, n - shared)])[p]
        Xc = X - np.array([0.4 * v, 0, 0])
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
        k = np.vstack([uv, np.stack([rng.uniform(0, W, n - shared), rng.uniform(0, H, n - shared)], 1)])[p]
        descs.append(np.ascontiguousarray(d)); kps.append(k.astype(np.float32))
    Rcw = np.tile(np.eye(3), (n_images, 1, 1))
    tcw = np.array([[-0.4 * v, 0, 0] for v in range(n_images)], np.float64)
    intr = intr.copy(); intr[4:] = 0.0
    return descs, kps, intr, Rcw, tcw, np.full((n_images, H, W), 8.0, np.float32)


def run(M, n_images, n, pairs, repeat, seed):
    V = importlib.import_module("global-lvba_amd.visual")
    descs, kps, intr, Rcw, tcw, planes = images(n_images, n, seed)
    out = {"n_images": n_images, "descriptors_per_image": n, "n_pairs": len(pairs)}
    with M.Matcher(descs) as m, V.DepthImages.upload(planes) as depth:
        m.set_geometry(kps, intr, Rcw, tcw)
        out["set_depth_ms"] = best_ms(lambda: m.set_depth(depth), repeat)
        for name, kw in (("unguided", {}), ("guided", {"guided": 1}), ("depth_guided", {"guided": 2}), ("unguided_one_sided", {"mutual": 0})):
            count = [0]

            def call():
                count[0] = m.match_pairs_csr(pairs, **kw)[3]
            ms = best_ms(call, repeat)
            scans = len(pairs) * (1 if kw.get("mutual") == 0 else 2)
            out[name] = {"ms": ms, "pairs_per_s": round(1e3 * len(pairs) / ms, 1), "tmacs": round(scans * n * n * 128 / ms * 1e-9, 3),
                         "matches": count[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--small", type=int, default=256)
    ap.add_argument("--small-pairs", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--oracle-size", type=int, default=2048)
    a = ap.parse_args()
    M = importlib.import_module("global-lvba_amd.match")
    res = {"few_large": [], "many_small": None}
    for n in a.sizes:
        pairs = np.array([(i, j) for i in range(4) for j in range(i + 1, 4)], np.int32)
        res["few_large"].append(run(M, 4, n, pairs, a.repeat, seed=n))
    k = 64
    rng = np.random.default_rng(0)
    allp = np.array([(i, j) for i in range(k) for j in range(i + 1, k)], np.int32)
    res["many_small"] = run(M, k, a.small, allp[rng.permutation(len(allp))[:a.small_pairs]], a.repeat, seed=1)
    if a.oracle_size:
        import match_oracle as mo
        descs = images(2, a.oracle_size, seed=a.oracle_size)[0]
        t0 = time.perf_counter()
        mo.match_pair(descs, 0, 1)
        res["oracle_ms"] = {"descriptors_per_image": a.oracle_size, "ms": round(1e3 * (time.perf_counter() - t0), 1),
                            "what": "numpy int64 matmul + arg-max, single thread, both directions"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
