"""Marginal pose covariance (lvba_balm_covariance) at a bench.py config (default C3: 2 000 poses x 10 M factors).

Refines the synthetic problem (the LM trace is reported), then times `--steps` covariance calls with an anchor: the
wall time per call, and the stage times the library prints under LVBA_TIMING=cov (HIP events: evaluation, one-ended
factorisation with its pivot test, selected inversion, gather + download).  Prints one JSON line.

    python tools/covariance_bench.py [--config C3] [--steps 10] [--warmup 2] [--anchor 0] [--host-inverse]

--host-inverse also times np.linalg.inv of the dense Hessian on the host (the comparison the covariance replaces)."""
import argparse
import importlib
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--anchor", type=int, default=0)
    ap.add_argument("--host-inverse", action="store_true")
    args = ap.parse_args()
    os.environ["LVBA_TIMING"] = "cov"
    import torch  # noqa: F401  (the HIP runtime torch brings, as bench.py loads it)
    pkg = importlib.import_module("global-lvba_amd")
    synth = importlib.import_module("global-lvba_amd.synth")
    N, V = synth.CONFIGS[args.config]
    d = synth.make_balm_problem(N, V, device="cuda:0")
    off = d["voxel_off"]
    p = pkg.BalmProblem(N, off, d["pose_idx"], d["clusters"])
    info = p.info()
    x, trace, rc = p.refine(d["poses_init"], max_iter=10)
    # the covariance is taken at the ground-truth poses: H is positive definite there once anchored (a refinement of the
    # synthetic problem can end beside a voxel whose lambda_min is not locally convex: H indefinite, the call refused)
    gt = d["poses_gt"]
    x = np.ascontiguousarray(gt.cpu().numpy() if hasattr(gt, "cpu") else gt, np.float64).reshape(-1, 12)
    stages, walls = [], []
    err = sys.stderr.fileno()
    with tempfile.TemporaryFile(mode="w+") as tf:
        saved = os.dup(err)
        os.dup2(tf.fileno(), err)
        try:
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                diag, _, _ = p.covariance(x, anchor=args.anchor)
                if k >= args.warmup:
                    walls.append((time.perf_counter() - t0) * 1e3)
        finally:
            os.dup2(saved, err)
            os.close(saved)
        tf.seek(0)
        for ln in tf.read().splitlines():
            m = re.search(r"lvba cov: eval ([\d.]+) ms factor ([\d.]+) ms selinv ([\d.]+) ms gather ([\d.]+) ms", ln)
            if m:
                stages.append([float(v) for v in m.groups()])
    st = np.array(stages[args.warmup:])
    med = np.median(st, axis=0) if len(st) else [float("nan")] * 4
    out = {"workload": f"{args.config}: {N} poses x {V} voxels x {int(off[-1])} factors", "n": 6 * N,
           "band_blocks": info["band_blocks"], "use_band": info["use_band"], "refine_rc": rc, "refine_iters": len(trace),
           "anchor": args.anchor, "steps": len(walls), "wall_ms_median": float(np.median(walls)), "wall_ms_min": float(np.min(walls)),
           "eval_ms": float(med[0]), "factor_ms": float(med[1]), "selinv_ms": float(med[2]), "gather_ms": float(med[3]),
           "diag_finite": bool(np.isfinite(diag).all())}
    if args.host_inverse:
        H, _, _ = p.eval(x, want_g=False)
        keep = np.ones(6 * N, bool)
        keep[6 * args.anchor:6 * args.anchor + 6] = False
        t0 = time.perf_counter()
        Hi = np.linalg.inv(H[np.ix_(keep, keep)])
        out["host_inv_ms"] = (time.perf_counter() - t0) * 1e3
        del Hi, H
    print(json.dumps(out))


if __name__ == "__main__":
    main()
