"""Cost of the LiDAR stage's robust loss itself: lvba_balm_eval and lvba_balm_cost on ONE handle of the headline problem with the loss
off, on (Cauchy), off, on, timed by the HIP events of lvba_balm_set_profiling.  The baseline is the loss-off timing of the same
handle in the same process; the off / off spread is the noise the on / off ratio has to be read against.  The scale is taken from
the handle's own lvba_balm_voxel_residuals at the initial poses (a^2 = 4 x the 90th percentile of lambda_min).
usage: python tools/loss_bench.py [calls per phase] [config]"""
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402

pkg = importlib.import_module("global-lvba_amd")
synth = importlib.import_module("global-lvba_amd.synth")


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    N, V = bench.parse_config(sys.argv[2] if len(sys.argv) > 2 else "C3", synth)
    d = synth.make_balm_problem(N, V, device="cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    x0 = np.asarray(d["poses_init"]).reshape(-1, 12)
    p = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"], device=0)
    lam, _ = p.voxel_residuals(x0)
    a = float(np.sqrt(4.0 * np.percentile(lam, 90)))
    p.set_profiling(True)
    phases = []
    for name, loss in (("warm-up", None), ("off", None), ("on", ("cauchy", a)), ("off", None), ("on", ("cauchy", a))):
        p.set_loss(loss)
        for _ in range(3):                       # the first calls after a switch are not timed
            p.eval(x0, want_H=False, want_g=False)
            p.cost(x0)
        p.profile(reset=True)
        for _ in range(calls):
            p.eval(x0, want_H=False, want_g=False)
        for _ in range(calls):
            c = p.cost(x0)
        pr = p.profile(reset=True)
        if name != "warm-up":
            phases.append(dict(loss=name, cost=c, eval_kernel_ms=pr["eval_kernel_ms"] / pr["eval_calls"],
                               cost_kernel_ms=pr["cost_kernel_ms"] / pr["cost_calls"], eval_ms=pr["eval_ms"] / pr["eval_calls"],
                               cost_ms=pr["cost_ms"] / pr["cost_calls"]))
    _, w = p.voxel_residuals(x0)                 # (the loss is on: the weights in effect)
    off = [q for q in phases if q["loss"] == "off"]
    on = [q for q in phases if q["loss"] == "on"]
    out = dict(config=[N, V], calls=calls, scale_m=a, down_weighted_share=float(np.mean(w < 0.5)), phases=phases)
    for k in ("eval_kernel_ms", "cost_kernel_ms"):
        m_off, m_on = np.mean([q[k] for q in off]), np.mean([q[k] for q in on])
        out[k] = dict(off=[q[k] for q in off], on=[q[k] for q in on], on_over_off=float(m_on / m_off),
                      off_off_spread=float(abs(off[0][k] - off[1][k]) / m_off))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
