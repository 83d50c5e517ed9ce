"""Pairwise consistency of loop closures (lvba_closure_consistency): timings at M closures on a synthetic multi-lap
trajectory, 10 % of the closures outliers in small mutually consistent groups.

    python tools/closure_bench.py [--closures 1000 4000 16000] [--group 5] [--seeds 32] [--repeat 5]

The library call is one: the pair pass is timed as the call with all four tolerances at zero -- the same M^2 cycles, an adjacency
that is the identity, every seed's candidate set empty, so that the set search has nothing to do -- and the set search as the full
call minus that.  Both include the upload of the closures and the download of keep (no adjacency, no diagnostics).  Host clock
around calls that end in a device synchronise, best of --repeat.  Per size the line also holds the model figures the timings are to be
read against: pairs, and the words the set search reads, sum over seeds and rounds of |C| W, counted by replaying the rule on the
adjacency the call returned.  Prints one JSON line.  Needs a HIP device."""
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


def rz(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([c, -s, z, s, c, z, z, z, o], -1).reshape(a.shape + (3, 3))


def trajectory(n):
    """Laps of 500 frames on a circle of radius 40 m, 1 m apart in height, heading along the tangent."""
    t = np.arange(n) * (2 * np.pi / 500)
    R = rz(t + 0.5 * np.pi)
    p = np.stack([40 * np.cos(t), 40 * np.sin(t), (np.arange(n) // 500).astype(float)], -1)
    return R, p


def closures(M, group, seed=0):
    """(poses [n,12], ref, query, meas [M,12], inlier mask): closure k ties frame i of lap 0 to the same place a lap later; every
    tenth run of `group` closures shares a world-frame discrepancy of its own (tens of metres: the bound grows to 10 m over the
    1 000 odometry steps two closures can be apart), the others agree with the poses to 1 mrad and 5 mm."""
    rng = np.random.default_rng(seed)
    n = 1000
    R, p = trajectory(n)
    i = rng.integers(0, 500, M)
    j = i + 500
    g = np.arange(M) // group
    out = g % 10 == 9
    Rd = np.where(out[:, None, None], rz(0.3 * rng.normal(size=M // group + 1))[g], np.eye(3))
    td = np.where(out[:, None], ((30.0 + 20.0 * rng.random((M // group + 1, 3))) * rng.choice([-1.0, 1.0], (M // group + 1, 3)))[g], 0.0)
    w = 1e-3 * rng.normal(size=(M, 3))
    K = np.zeros((M, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    Rn = np.eye(3) + K + 0.5 * K @ K
    u, _, vt = np.linalg.svd(Rn)
    Rn, tn = u @ vt, 5e-3 * rng.normal(size=(M, 3))
    # Z = X_i^-1 D^-1 X_j N
    Ra = np.swapaxes(R[i], 1, 2) @ np.swapaxes(Rd, 1, 2)                         # R_i^T R_d^T
    ta = np.einsum("kab,kb->ka", Ra, -td) - np.einsum("kba,kb->ka", R[i], p[i])  # of X_i^-1 D^-1
    Rb = Ra @ R[j]
    tb = np.einsum("kab,kb->ka", Ra, p[j]) + ta
    Rz_, tz = Rb @ Rn, np.einsum("kab,kb->ka", Rb, tn) + tb
    poses = np.concatenate([R.reshape(n, 9), p], 1)
    return poses, i.astype(np.int32), j.astype(np.int32), np.concatenate([Rz_.reshape(M, 9), tz], 1), ~out


def words_read(words, n_seeds):
    """The rule replayed on the adjacency (rows as Python integers), early exit included: (sum over seeds and rounds of |C| W,
    rounds per seed)."""
    M, W = words.shape
    rows = [int.from_bytes(words[a].tobytes(), "little") for a in range(M)]
    pop = lambda s: bin(s).count("1")
    deg = [pop(r) - 1 for r in rows]
    seeds = sorted(range(M), key=lambda v: (-deg[v], v))[:min(n_seeds, M)]
    total, rounds = 0, []
    for s in seeds:
        C, r = rows[s] & ~(1 << s), 0
        while C:
            r += 1
            size, best, full = pop(C), None, True
            total += size * W
            rest = C
            while rest:
                low = rest & -rest
                v = low.bit_length() - 1
                rest ^= low
                c = pop(rows[v] & C)
                full = full and c == size
                if best is None or c > best[0]:
                    best = (c, v)
            if full:
                break
            C = C & rows[best[1]] & ~(1 << best[1])
        rounds.append(r)
    return total, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--closures", type=int, nargs="*", default=[1000, 4000, 16000])
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="skip the replay of the rule on the host")
    a = ap.parse_args()
    pkg = importlib.import_module("global-lvba_amd")
    reg = importlib.import_module("global-lvba_amd.register")
    L = pkg._lib
    lib = L.load()
    if lib.lvba_device_count() < 1:
        raise SystemExit("closure_bench needs a HIP device")
    import ctypes as C
    out = dict(bench="closure", group=a.group, n_seeds=a.seeds, sizes=[])
    for M in a.closures:
        poses, ref, query, meas, inlier = closures(M, a.group)
        keep, n_keep = np.zeros(M, np.uint8), C.c_int32()

        def call(o):
            L.check(lib.lvba_closure_consistency(0, len(poses), poses.ctypes.data, M, ref.ctypes.data, query.ctypes.data, meas.ctypes.data,
                                                 C.byref(o), None, None, None, keep.ctypes.data, C.byref(n_keep)))
        full = L.ClosureOpts()
        lib.lvba_closure_default_opts(C.byref(full))
        full.n_seeds = a.seeds
        pairs_only = L.ClosureOpts(0.0, 0.0, 0.0, 0.0, a.seeds, 2)
        t_all, t_pair = best_ms(lambda: call(full), a.repeat), best_ms(lambda: call(pairs_only), a.repeat)
        call(full)
        row = dict(closures=M, pairs=M * M, kept=int(n_keep.value), inliers=int(inlier.sum()), kept_are_the_inliers=bool((keep.astype(bool) == inlier).all()),
                   total_ms=t_all, pair_pass_ms=t_pair, set_search_ms=round(t_all - t_pair, 3))
        if not a.no_model:
            got = reg.closure_consistency(poses, ref, query, meas, n_seeds=a.seeds)
            row["set_words_read"], rounds = words_read(got["words"], a.seeds)
            row["rounds_per_seed"] = [min(rounds), max(rounds)]
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
