"""ms per LM iteration of the headline problem with and without pose priors, interleaved in one process: a RELATIVE prior between
every pair of consecutive poses, a POSE prior on pose 0 and a POSITION prior (lever arm) on every 10th pose.
usage: python tools/prior_bench.py [rounds] [steps] [config]"""
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402

pkg = importlib.import_module("global-lvba_amd")
synth = importlib.import_module("global-lvba_amd.synth")


def priors_for(x):
    N = x.shape[0]
    P = pkg.Prior
    out = [P.pose(0, x[0], sigma_rot=1e-3, sigma_pos=1e-2)]
    for i in range(N - 1):
        Ri, Rj = x[i, :9].reshape(3, 3), x[i + 1, :9].reshape(3, 3)
        out.append(P.relative(i, i + 1, (Ri.T @ Rj, Ri.T @ (x[i + 1, 9:] - x[i, 9:])), sigma_rot=2e-3, sigma_pos=2e-2))
    arm = np.array([0.2, 0.0, 1.5])
    for i in range(0, N, 10):
        out.append(P.position(i, x[i, :9].reshape(3, 3) @ arm + x[i, 9:], sigma=0.05, lever_arm=arm))
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    N, V = bench.parse_config(sys.argv[3] if len(sys.argv) > 3 else "C3", synth)
    d = synth.make_balm_problem(N, V, device="cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    x0 = np.asarray(d["poses_init"]).reshape(-1, 12)
    gt = np.asarray(d["poses_gt"]).reshape(-1, 12)
    probs = {}
    for name in ("plain", "priors"):
        p = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"], device=0)
        if name == "priors":
            p.set_priors(priors_for(gt))
        p.refine(x0, max_iter=3)  # set-up, graph capture, warm caches
        probs[name] = p
    info = {k: p.info() for k, p in probs.items()}

    def run(p):
        p.lm_begin(x0, max_iter=steps, rel_tol=0.0)
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while True:
            row, done, rc = p.lm_step()
            n += 1
            evals[p] = evals.get(p, 0) + row["evaluated"]
            if done or rc != 0:
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        p.lm_end(want_poses=False)
        return 1e3 * dt / n

    ms = {k: [] for k in probs}
    evals = {}
    for _ in range(rounds):
        for k, p in probs.items():
            ms[k].append(run(p))
    print(json.dumps({"config": [N, V], "n_priors": len(priors_for(gt)), "steps": steps, "rounds": rounds,
                      "ms_per_iter": {k: sorted(v) for k, v in ms.items()},
                      "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
                      # iterations that evaluated H and g (the rest costed a trial point after a rejected step): the two runs need
                      # not take the same accept / reject path
                      "evaluated_fraction": {k: evals.get(p, 0) / float(rounds * steps) for k, p in probs.items()},
                      "band_blocks": {k: v["band_blocks"] for k, v in info.items()},
                      "nd_arcs": {k: v["nd_arcs"] for k, v in info.items()}}))


if __name__ == "__main__":
    main()
