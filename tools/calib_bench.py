"""Extrinsic-refinement timings: what one Gauss-Newton iteration of lvba_calib_extrinsic costs per record, beside a device copy of
the same bytes in the same run.

    python tools/calib_bench.py [--records 100000 1000000 10000000] [--jobs 1 8] [--repeat 5] [--iterations 10 510]
                                [--time-offset] [--out FILE]

Prints one JSON line.  An iteration is one launch of calib_linearize_kernel (grid (workgroups, jobs)), one of calib_step_kernel and
one synchronise; it reads 44 bytes per record per job (pair 4, target 16, point 24).  The call also uploads the records and
undistorts them, so an iteration's time is taken as a difference: the host clock around two calls that end in a device synchronise,
one of --iterations[0] and one of --iterations[1] iterations (eps_rot = eps_trans = 0 on noisy records: no job ever converges, every
call runs to its limit), best of --repeat each after a warm-up, divided by the difference in iterations.  "iter_ms" is that;
"read_gbs" = 44 n jobs / iter_ms, the rate at which the iteration consumes its records (for jobs > 1 the same records are read by
every job: the rate is what the caches deliver, not HBM traffic).  "copy_gbs": a device-to-device copy (torch, timed by device
events, best of --repeat after a warm-up) of a buffer of 44 n bytes, counted as read plus write, 88 n bytes.  "share_of_copy" =
read_gbs / copy_gbs for jobs = 1: the share of the bandwidth a plain copy reaches on this device in this run that the iteration
reaches.  The kernels' own times come from a run under `rocprofv3 --kernel-trace --stats`.  --time-offset: every (records, jobs)
entry gains "td", the same measurement of lvba_calib_extrinsic_td (calib_td_pairs_kernel, calib_td_linearize_kernel,
calib_td_step_kernel; 39 sums instead of 31 and one more small launch) over the same records with seeded twists, in the same run,
and "td_over_6" = its iter_ms over the 6-parameter iter_ms.  --out FILE also writes the JSON there.  Needs a HIP device."""
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

BYTES_PER_RECORD = 44


def best_ms(fn, repeat):
    fn()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms)


def copy_gbs(torch, nbytes, repeat):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.random_(0, 255)
    dst.copy_(src)
    torch.cuda.synchronize()
    best = None
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / 4
        best = ms if best is None else min(best, ms)
    return 2.0 * nbytes / (best * 1e6), best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[100000, 1000000, 10000000])
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iterations", type=int, nargs=2, default=[10, 510])
    ap.add_argument("--time-offset", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch                                                                  # first: its HIP runtime must be the process's
    L = importlib.import_module("global-lvba_amd._lib")
    if L.load().lvba_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("calib_bench needs a HIP device")
    CB = importlib.import_module("global-lvba_amd.calib")
    import calib_cases as cc
    import calib_oracle as co
    base = cc.make("general", M=10, per_pair=(min(max(args.records), 1000000) + 33) // 34, span=2, seed=21, noise_px=0.5, outliers=0.2)
    out = dict(bytes_per_record=BYTES_PER_RECORD, iterations=args.iterations, sizes=[])
    if args.time_offset:
        import calib_td_cases as tc
        twists = tc.seeded_twists("general", base["poses"], np.random.default_rng(22))
    k0, k1 = args.iterations
    for n in args.records:
        rep = max(1, (n + len(base["pair"]) - 1) // len(base["pair"]))
        take = (n + rep - 1) // rep
        idx = np.repeat(np.arange(take), rep)[:n]                                # a record repeated stays in its pair's run
        rec = dict(pair=np.ascontiguousarray(base["pair"][idx]), uv=np.ascontiguousarray(base["uv"][idx]),
                   Xb=np.ascontiguousarray(base["Xb"][idx]))
        table = (base["img_a"], base["img_b"])
        gbs, copy_ms = copy_gbs(torch, BYTES_PER_RECORD * n, args.repeat)
        row = dict(records=n, copy_ms=round(copy_ms, 4), copy_gbs=round(gbs, 1), jobs=[])
        for J in args.jobs:
            R = np.array([co.perturb(base["R_true"], base["t_true"], 0.01 * (j + 1) * np.r_[1, -1, 1, 1, 1, -1.0])[0] for j in range(J)])
            t = np.array([co.perturb(base["R_true"], base["t_true"], 0.01 * (j + 1) * np.r_[1, -1, 1, 1, 1, -1.0])[1] for j in range(J)])
            run = lambda k: CB.refine_jobs(rec, table, base["poses"], base["intr"], R, t, max_iterations=k, eps_rot=0.0, eps_trans=0.0)
            done = run(k1)
            assert (done["iterations"] == k1).all() and (done["status"] == CB.MAX_ITERATIONS).all(), (done["iterations"], done["status"])
            ms0, ms1 = best_ms(lambda: run(k0), args.repeat), best_ms(lambda: run(k1), args.repeat)
            it = (ms1 - ms0) / (k1 - k0)
            read = BYTES_PER_RECORD * n * J / (it * 1e6)
            e = dict(jobs=J, call_ms=[round(ms0, 3), round(ms1, 3)], iter_ms=round(it, 4), read_gbs=round(read, 1),
                     ns_per_record_job=round(1e6 * it / (n * J), 4))
            if J == 1:
                e["share_of_copy"] = round(read / gbs, 3)
            if args.time_offset:
                run_td = lambda k: CB.refine_jobs_td(rec, table, base["poses"], twists, base["intr"], R, t, 0.0, max_iterations=k, eps_rot=0.0,
                                                     eps_trans=0.0, eps_td_s=0.0)
                done = run_td(k1)
                assert (done["iterations"] == k1).all() and (done["status"] == CB.MAX_ITERATIONS).all(), (done["iterations"], done["status"])
                td0, td1 = best_ms(lambda: run_td(k0), args.repeat), best_ms(lambda: run_td(k1), args.repeat)
                it_td = (td1 - td0) / (k1 - k0)
                e["td"] = dict(call_ms=[round(td0, 3), round(td1, 3)], iter_ms=round(it_td, 4),
                               read_gbs=round(BYTES_PER_RECORD * n * J / (it_td * 1e6), 1), ns_per_record_job=round(1e6 * it_td / (n * J), 4))
                e["td_over_6"] = round(it_td / it, 3)
            row["jobs"].append(e)
        out["sizes"].append(row)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
