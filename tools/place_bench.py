"""Place-recognition timings: the descriptor pass (lvba_place_descriptors) on synthetic scans and the search
(lvba_place_search) on synthetic descriptors.

    python tools/place_bench.py [--scan-frames 64] [--points 100000] [--frames 2000 10000] [--repeat 5]

Prints one JSON line (host clock around calls that end in a device synchronise, best of --repeat; the descriptor call includes
the copy of the descriptors to the host, the search call the copy of the descriptors to the device).  Needs a HIP device."""
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


def descriptors(n, nr=20, ns=60, seed=1):
    """n descriptors: laps of 500 places, every lap the same images turned by a sector per lap with a tenth of the cells redrawn."""
    rng = np.random.default_rng(seed)
    base = (rng.random((500, nr, ns)) * 4.0).astype(np.float32)
    base[rng.random(base.shape) < 0.4] = 0.0
    out = np.zeros((n, nr, ns), np.float32)
    for f in range(n):
        img = np.roll(base[f % 500], f // 500, axis=1)
        redraw = rng.random((nr, ns)) < 0.1
        out[f] = np.where(redraw, (rng.random((nr, ns)) * 4.0).astype(np.float32), img)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--frames", type=int, nargs="*", default=[2000, 10000])
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("global-lvba_amd")
    synth = importlib.import_module("global-lvba_amd.synth")
    reg = importlib.import_module("global-lvba_amd.register")
    if pkg._lib.load().lvba_device_count() < 1:
        raise SystemExit("place_bench needs a HIP device")
    out = dict(bench="place", search=[])
    if a.scan_frames > 0:
        s = synth.make_scans(a.scan_frames, a.points, seed=5, noise=0.005, clutter_frac=0.05)
        with pkg.Scans(s["clouds"]) as sc:
            ms = best_ms(lambda: reg.scan_descriptors(sc, max_range=40.0), a.repeat)
        pts = int(sum(len(c) for c in s["clouds"]))
        out["descriptors"] = dict(frames=a.scan_frames, points=pts, ms=ms, gb_per_s=round(12e-6 * pts / ms, 1))
    for n in a.frames:
        d = descriptors(n)
        got = reg.place_search(d)
        out["search"].append(dict(frames=n, count=got["count"], ms=best_ms(lambda: reg.place_search(d), a.repeat)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
