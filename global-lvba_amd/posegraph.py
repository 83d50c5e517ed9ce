"""Pose-graph relaxation over odometry and loop closures (lvba_posegraph_relax; include/lvba_hip.h has the problem and the LM rule,
DESIGN.md §10g the kernels)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

POSEGRAPH_OPTS = L.option_names(L.PosegraphOpts) + ("closure_loss",)


def posegraph_opts(**opts):
    """An lvba_posegraph_opts with the library's defaults and `opts` on top; closure_loss is a (kind, scale) pair or None."""
    opts = dict(opts)
    given, loss = "closure_loss" in opts, opts.pop("closure_loss", None)
    o = L.make_opts(L.PosegraphOpts, "pose-graph", ("closure_loss",), **opts)
    if given:                               # None here means TRIVIAL, not "keep the default" (register's loss differs)
        o.closure_loss = L.Loss(0, 0, 0.0) if loss is None else L.loss_struct(loss).contents
    return o


def relax_pose_graph(poses, priors, device=0, **opts):
    """Relax the trajectory `poses` [n,12] over its own odometry (the relative motion of consecutive input poses) and the loop
    closures `priors` (balm.Prior.relative objects, as pipeline.find_loop_closures returns them), pose `anchor` held in place.
    opts: POSEGRAPH_OPTS.  Returns dict(poses [n,12], weights [len(priors)] = rho' of every closure at the result, report,
    trace = one dict per LM iteration).  A numerical status (LVBA_NUM_*) is in report["status"], not raised."""
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    priors = list(priors)
    o = posegraph_opts(**opts)
    arr = (L.Prior * max(1, len(priors)))(*priors)
    out, w = np.zeros_like(x), np.zeros(len(priors))
    trace, n_trace, rep = (L.LmTrace * max(1, int(o.max_iter)))(), C.c_int32(0), L.PosegraphReport()
    lib = L.load()
    L.check(lib.lvba_posegraph_relax(len(x), x.ctypes.data, len(priors), C.cast(arr, C.c_void_p) if priors else None, C.byref(o),
                                     int(device), out.ctypes.data, w.ctypes.data if priors else None, C.cast(trace, C.c_void_p),
                                     C.byref(n_trace), C.byref(rep)), allow_numeric=True)
    r = rep.as_dict()
    r["solver"] = L.PG_SOLVER_KINDS.get(r["solver_kind"], "?")
    return dict(poses=out, weights=w, report=r, trace=[trace[k].as_dict() for k in range(n_trace.value)])
