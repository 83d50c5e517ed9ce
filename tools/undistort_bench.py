"""Times the kernel of the undistorted-image export (lvba_undistort_images, csrc/undistort.hip) for 64 and 256
images of 1 280 x 1 024 at the reference's defaults (same size, newK = K), plain and with exposure gains.  Beside it, in the same
run and alternating with it repetition by repetition: a device-to-device copy that reads and writes as many bytes as the kernel
reads and writes at the least (the input images plus the output images), and once, on one image, the numpy oracle of the tests.
No test runs this.  The numbers go into DESIGN.md §10s and a JSON file:

    python tools/undistort_bench.py --out profiles/undistort_bench.json [--images 64 256] [--reps 5]

Kernel times are the library's own device events around the launch (lvba_undistort_profile), one launch per call
(max_batch_images = 0); the copy is timed with device events around torch's copy_.  Every shape is warmed up once."""
import argparse
import importlib
import json
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

W, H = 1280, 1024
INTR = np.array([1210.0, 1208.0, 642.3, 509.6, -0.076160, 0.123001, -0.00113, 0.000251])   # the reference camera's distortion


def stats(v):
    return dict(mean=sum(v) / len(v), min=min(v), max=max(v))


def copy_ms(n_bytes):
    """device ms of one device-to-device copy of n_bytes (it reads n_bytes and writes n_bytes)"""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return float(e0.elapsed_time(e1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    UN = importlib.import_module("global-lvba_amd.undistort")
    if importlib.import_module("global-lvba_amd._lib").load().lvba_device_count() < 1 or torch is None or not torch.cuda.is_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    import undistort_oracle as uo
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    want = uo.images(base[:1], INTR)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    rows = []
    for M in a.images:
        images = np.ascontiguousarray(base[np.arange(M) % len(base)])
        gains = np.zeros((M, 3, 2), np.int64)
        gains[:, :, 0] = rng.integers(int(0.8 * 65536), int(1.25 * 65536), (M, 3))
        gains[:, :, 1] = rng.integers(-5 * 256 * 65536, 5 * 256 * 65536, (M, 3))
        t = dict(plain=[], gains=[], copy=[])
        with UN.Undistorter(INTR, W, H, max_batch_images=0) as und:
            traffic = images.nbytes + M * und.size[0] * und.size[1] * 3       # bytes read plus bytes written, at the least
            before = 0.0
            for r in range(a.reps + 1):                                        # round 0 warms every pass up
                for name, g in (("plain", None), ("gains", gains)):
                    out = und.images(images, gains=g)
                    now = und.profile()["kernel"]
                    if r:
                        t[name].append(now - before)
                    before = now
                    if r == 0 and g is None:
                        assert out[0].tobytes() == want[0].tobytes()           # what is timed is the rule
                ms = copy_ms(traffic // 2)
                if r:
                    t["copy"].append(ms)
            prof, n_valid, size = und.profile(), und.n_valid, und.size
        s = {k: stats(v) for k, v in t.items()}
        row = dict(n_images=M, width=W, height=H, out_width=size[0], out_height=size[1], n_valid=n_valid, reps=a.reps, traffic_bytes=traffic,
                   plain_ms=s["plain"], gains_ms=s["gains"], copy_ms=s["copy"],
                   plain_gbytes_per_s=traffic / (s["plain"]["mean"] * 1e-3) / 1e9, gains_gbytes_per_s=traffic / (s["gains"]["mean"] * 1e-3) / 1e9,
                   copy_gbytes_per_s=traffic / (s["copy"]["mean"] * 1e-3) / 1e9,
                   plain_share_of_copy=s["copy"]["mean"] / s["plain"]["mean"], gains_share_of_copy=s["copy"]["mean"] / s["gains"]["mean"],
                   pixels_per_s=M * size[0] * size[1] / (s["plain"]["mean"] * 1e-3),
                   upload_ms_total=prof["upload"], download_ms_total=prof["download"], oracle_one_image_ms=oracle_ms,
                   kernel_one_image_ms=s["plain"]["mean"] / M)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(tool="tools/undistort_bench.py", options="defaults, max_batch_images=0", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
