"""Track-building timings: trackgraph.TrackGraph (create = the graph, its components and the two size checks; orders = the BFS
order of every component with its uv) on synthetic match sets, beside the host mirror pipeline.build_components and beside the
compiled C++ loop of include/lvba_adapter.hpp (tools/adapter_tracks_bench.cpp, when it has been built).

    python tools/tracks_bench.py [--sizes 64:200000 256:2000000 1024:20000000] [--giant 256:2000000:100000] [--repeat 3]
                                 [--host-up-to 2000000] [--no-host] [--no-adapter] [--scratch DIR]

Prints one JSON line.  A match set: tracks of 5 views over consecutive images (all 10 view pairs of a track are matches, so a set of
m matches has m / 10 tracks over the pairs (i, i + 1 .. i + 4)), key point indices shuffled inside every image; --giant adds a
planted component of about that many nodes (tracks linked into one chain by further matches).  Times are the host clock around
calls that end in a device synchronise, best of --repeat after a warm-up, uploads and downloads included: create_ms is
TrackGraph(keypoints, pairs, matches) from the per-pair arrays the matcher returns, orders_ms is .orders(uv=True) of all
components.  host_ms is pipeline.build_components on the same input, once, on this machine's CPU.  adapter_ms is
build_tracks_and_fuse_with with a fusion that accepts everything (best of --repeat, the match table already in the reference's
form).  The kernels' own times come from a run under `rocprofv3 --kernel-trace --stats` with --no-host --no-adapter.  Needs a HIP
device."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ADAPTER = os.path.join(ROOT, "tools", "adapter_tracks_bench")
VIEWS = 5


def best_ms(fn, repeat):
    fn()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(min(ms), 3)


def match_set(M, n_matches, giant=0, seed=5):
    """(keypoints: float32 [n_i, 2] per image, pairs: [(i, j)], matches: int32 [m, 2] per pair)"""
    rng = np.random.default_rng(seed)
    T = n_matches // (VIEWS * (VIEWS - 1) // 2)
    first = rng.integers(0, M - VIEWS + 1, T)
    img = (first[:, None] + np.arange(VIEWS)[None, :]).reshape(-1)                 # observation o = VIEWS t + v
    order = np.lexsort((rng.random(len(img)), img))                                # by image, shuffled inside it
    counts = np.bincount(img, minlength=M)
    start = np.concatenate([[0], np.cumsum(counts)])
    kp = np.empty(len(img), np.int64)
    kp[order] = np.arange(len(img)) - start[img[order]]
    a, b = np.triu_indices(VIEWS, 1)
    oa, ob = (VIEWS * np.arange(T)[:, None] + a[None, :]).reshape(-1), (VIEWS * np.arange(T)[:, None] + b[None, :]).reshape(-1)
    if giant:
        link = np.sort(rng.choice(T, giant // VIEWS, replace=False))               # track k's first view to track k + 1's last
        xa, xb = VIEWS * link[:-1], VIEWS * link[1:] + VIEWS - 1
        xb = np.where(img[xa] == img[xb], xb - 1, xb)                               # ... or its last but one, where the images coincide
        swap = img[xa] > img[xb]
        xa, xb = np.where(swap, xb, xa), np.where(swap, xa, xb)
        oa, ob = np.concatenate([oa, xa]), np.concatenate([ob, xb])
    pair_key = img[oa] * M + img[ob]
    by_pair = np.argsort(pair_key, kind="stable")
    keys, where = np.unique(pair_key[by_pair], return_index=True)
    rows = np.stack([kp[oa[by_pair]], kp[ob[by_pair]]], 1).astype(np.int32)
    matches = np.split(rows, where[1:])
    pairs = [(int(k // M), int(k % M)) for k in keys]
    kps = [rng.uniform(0, 640, (int(n), 2)).astype(np.float32) for n in counts]
    return kps, pairs, matches


def adapter_ms(kps, pairs, matches, repeat, scratch):
    """the compiled C++ loop on the same input, through a file of int64 / float32 words"""
    path = os.path.join(scratch, "tracks_bench_input.bin")
    with open(path, "wb") as f:
        np.array([len(kps), len(pairs), repeat], np.int64).tofile(f)
        np.array([len(k) for k in kps], np.int64).tofile(f)
        np.asarray(pairs, np.int64).reshape(-1).tofile(f)
        np.concatenate([[0], np.cumsum([len(m) for m in matches])]).astype(np.int64).tofile(f)
        np.concatenate(matches).astype(np.int32).tofile(f)
        np.concatenate(kps).astype(np.float32).tofile(f)
    try:
        return json.loads(subprocess.check_output([ADAPTER, path], text=True))
    finally:
        os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["64:200000", "256:2000000", "1024:20000000"])
    ap.add_argument("--giant", nargs="*", default=["256:2000000:100000"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-up-to", type=int, default=2_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-adapter", action="store_true")
    ap.add_argument("--scratch", default=tempfile.gettempdir())
    args = ap.parse_args()
    L = importlib.import_module("global-lvba_amd._lib")
    if L.load().lvba_device_count() < 1:
        raise SystemExit("tracks_bench needs a HIP device")
    TG = importlib.import_module("global-lvba_amd.trackgraph")
    pl = importlib.import_module("global-lvba_amd.pipeline")
    out = dict(views=VIEWS, obser_thr=3, library=os.path.basename(L.LIB_PATH), sizes=[])
    for spec in list(args.sizes) + list(args.giant):
        M, n_matches, giant = (list(map(int, spec.split(":"))) + [0])[:3]
        kps, pairs, matches = match_set(M, n_matches, giant)
        row = dict(images=M, pairs=len(pairs), matches=int(sum(len(m) for m in matches)), planted=giant)
        graphs = []

        def create():
            while graphs:
                graphs.pop().close()
            graphs.append(TG.TrackGraph(kps, pairs, matches, 3))

        row["create_ms"] = best_ms(create, args.repeat)
        g = graphs[0]
        g.components()
        row.update(g.info)
        row["orders_ms"] = best_ms(lambda: g.orders(uv=True), args.repeat)
        got = g.orders()
        if not args.no_host and row["matches"] <= args.host_up_to:
            t0 = time.perf_counter()
            want = pl.build_components([len(k) for k in kps], pairs, matches, 3)
            row["host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            row["host_equal"] = all(np.array_equal(x, y) for x, y in zip(got, want))
        if not args.no_adapter and os.path.exists(ADAPTER):
            res = adapter_ms(kps, pairs, matches, args.repeat, args.scratch)
            row["adapter_ms"] = res["ms"]
            row["adapter_equal"] = res["tracks"] == row["n_components"] and res["observations"] == row["n_observations"] and \
                res["checksum"] == int((got[1].astype(np.int64) * 1000003 + got[2]).sum() % (2 ** 61 - 1))
        g.close()
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
