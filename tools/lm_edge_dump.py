#!/usr/bin/env python3
"""Every output of a fixed list of small calls whose arithmetic runs through the LM damping rule (csrc/lm_rule.h) and the prior
edge's record (csrc/prior_device.h), into one .npz -- for a byte comparison of two builds of the library (the kernels are
deterministic: two runs of one build give the same bytes).

    python tools/lm_edge_dump.py OUT.npz [--call NAME ...]       # needs a GPU; LVBA_HIP_LIB selects the build
    python tools/lm_edge_dump.py --compare A.npz B.npz           # exit status 1 unless every array is byte-equal

The calls (problems of the GPU tests, imported from tests/):
    posegraph   lvba_posegraph_relax on posegraph_cases' pair, ring64, lever and cauchy: poses, weights, trace, report
    priors      lvba_balm_refine, lvba_balm_prior_residuals and lvba_balm_eval_blocks with test_gpu_priors' mixed priors
    visual      lvba_visual_refine (and cost, linearize) with test_gpu_visual_priors' mixed priors on its smallest case
    window      lvba_window_ba on the problem of test_windows_in_lock_step_equal_one_at_a_time (the grouped rule)
    reject      lvba_balm_refine on tests/golden/balm_reject.npz (a trace with rejected steps)
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def flatten(out, name, v):
    """numbers, arrays and nests of dicts / sequences of them -> out[name/...] arrays (a dict's keys in sorted order)"""
    if isinstance(v, dict):
        for k in sorted(v):
            flatten(out, f"{name}/{k}", v[k])
    elif isinstance(v, (list, tuple)) and not all(isinstance(x, (int, float, bool, np.number)) for x in v):
        out[f"{name}/len"] = np.array(len(v))
        for k, x in enumerate(v):
            flatten(out, f"{name}/{k}", x)
    elif isinstance(v, str) or v is None:
        out[name] = np.array(str(v))
    else:
        out[name] = np.asarray(v)


def call_posegraph(pkg, out):
    import posegraph_cases as pgc
    from test_gpu_posegraph import run
    pgm = importlib.import_module("global-lvba_amd.posegraph")
    for name in ("pair", "ring64", "lever", "cauchy"):
        flatten(out, f"posegraph/{name}", run(pgm, pgc.named(name)))


def call_priors(pkg, out):
    import test_gpu_priors as tp
    from conftest import make_problem
    d = make_problem(**tp.BAND)
    p = tp._prob(pkg, d, tp._mix(d))
    x = d["poses_init"]
    flatten(out, "priors/eval_blocks", p.eval_blocks(x))
    flatten(out, "priors/prior_residuals", p.prior_residuals(x))
    flatten(out, "priors/refine", p.refine(x))


def call_visual(pkg, out):
    import test_gpu_visual_priors as tv
    import visual_prior_cases as vc
    synth = importlib.import_module("global-lvba_amd.synth")
    d, prob, _ = tv._mk(pkg, synth, tv.SMALL)
    prob.set_priors(vc.mixed_priors(synth, d))
    flatten(out, "visual/prior_residuals", prob.prior_residuals(d["q"], d["t"]))
    flatten(out, "visual/run_all", tv._run_all(prob, d))
    prob.close()


def call_window(pkg, out):
    synth = importlib.import_module("global-lvba_amd.synth")
    s = synth.make_scans(22, 6000, room=(10, 8, 4), origin=(2.0, -1.0, 0.4), n_panels=8, seed=43, rot_sigma_deg=0.1, trans_sigma=0.03)
    clouds = [c.copy() for c in s["clouds"]]
    for f in range(8, 12):
        clouds[f] = clouds[f][:40]
    with pkg.Scans(clouds) as scans:
        got = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, anchor_leaf=0.05, lm_mode=0)
    asc = got.pop("anchor_scans")
    for w in got["windows"]:                     # wall-clock times are no outputs
        for k in [k for k in w if k.endswith("_ms")]:
            del w[k]
    flatten(out, "window/anchor_clouds", [asc.download(a) for a in range(len(got["anchor_poses"]))])
    asc.close()
    flatten(out, "window/out", got)


def call_reject(pkg, out):
    z = np.load(os.path.join(ROOT, "tests", "golden", "balm_reject.npz"))
    prob = pkg.BalmProblem(int(z["n_poses"]), z["voxel_off"], z["pose_idx"], z["clusters"])
    flatten(out, "reject/refine", prob.refine(z["poses_init"]))


CALLS = dict(posegraph=call_posegraph, priors=call_priors, visual=call_visual, window=call_window, reject=call_reject)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"only in one file: {k}")
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        if x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes():
            continue
        bad.append(k)
        if x.shape == y.shape and x.dtype.kind == "f":
            with np.errstate(all="ignore"):
                r = np.nanmax(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))
            print(f"DIFFERENT {k}: largest relative difference {r:.3e}")
        else:
            print(f"DIFFERENT {k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}")
    print(f"{len(set(A.files) & set(B.files))} arrays in both, {len(bad)} not byte-equal")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--call", action="append", choices=sorted(CALLS), help="only these calls (default: all)")
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    if a.compare:
        if len(a.paths) != 2:
            ap.error("--compare takes two files")
        return compare(*a.paths)
    if len(a.paths) != 1:
        ap.error("one output file")
    pkg = importlib.import_module("global-lvba_amd")
    out = {}
    for name in a.call or list(CALLS):
        CALLS[name](pkg, out)
        print(f"{name}: {len(out)} arrays so far", flush=True)
    np.savez(a.paths[0], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
