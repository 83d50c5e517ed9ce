"""The shared loop-closure fixture of tests/test_loop_host.py and tests/test_gpu_loop.py, computed once per process.

make_scans(12, 3000, room=(8, 6, 3)) flies one closed loop: frame 11 neighbours frame 0.  Submaps of 3 frames, min_gap 6.
RADIUS admits the last frames against the first submap and the first frames against the last one and nothing across the room;
RADIUS_WIDE lets a second, farther submap in for some queries, so that max_per_frame = 1 has something to cut.  The end-to-end
case starts from poses_gt with a drift that grows linearly with the frame index to DRIFT_ROT / DRIFT_TRANS at frame 11.  The
study behind these values is DESIGN.md §10d.

LAPS is a poses-only case for the candidate search alone: three laps on a coarse grid, so that queries have several eligible
submaps, exact ties between frames and between submaps occur, and more than one workgroup runs.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np

from oracle import voxel_oracle as vo
import loop_oracle as lo
import register_oracle as ro

VS = 1.0
RATIO = np.float32([0.02, 0.02, 0.02, 0.02])
NOISE = 0.005
N, S, MIN_GAP = 12, 3, 6
RADIUS, RADIUS_WIDE = 2.5, 3.7
SEARCH = dict(submap_size=S, min_gap=MIN_GAP, max_per_frame=2, query_stride=1, radius=RADIUS)
OPTS = dict(max_iterations=30, max_distance=0.1, min_inliers=100, min_eigenvalue=1e-3, tol_rot=1e-6, tol_pos=1e-6)
DRIFT_ROT, DRIFT_TRANS, DRIFT_SEED = np.radians(1.5), 0.08, 1
ACCEPT = dict(min_inlier_frac=0.3, max_rmse=0.03, max_rot=np.radians(5.0), max_trans=0.5)


@functools.lru_cache(maxsize=None)
def scans():
    synth = importlib.import_module("global-lvba_amd.synth")
    return synth.make_scans(N, 3000, room=(8, 6, 3), origin=(2.5, -1.5, 0.2), n_panels=6, seed=5, noise=NOISE, clutter_frac=0.05)


def truth():
    return scans()["poses_gt"].copy()


@functools.lru_cache(maxsize=None)
def _drifted():
    rng = np.random.default_rng(DRIFT_SEED)
    ax, dt = rng.normal(size=3), rng.normal(size=3)
    ax, dt = ax / np.linalg.norm(ax), dt / np.linalg.norm(dt)
    P = truth()
    return np.stack([ro.retract(P[f], np.r_[DRIFT_ROT * ax, DRIFT_TRANS * dt] * (f / (N - 1))) for f in range(N)])


def drifted():
    return _drifted().copy()


def poses(which):
    return {"truth": truth, "drifted": drifted}[which]()


def submap_frames(w, n=N, s=S):
    return range(w * s, min((w + 1) * s, n))


@functools.lru_cache(maxsize=None)
def oracle_submap(which, w):
    """The oracle's plane map of submap w at the poses `which`."""
    P, fr = poses(which), submap_frames(w)
    surf, _ = vo.build([scans()["clouds"][f][:, :3] for f in fr], P[fr.start:fr.stop], VS, RATIO)
    return surf


@functools.lru_cache(maxsize=None)
def candidates(which):
    return lo.candidates(poses(which), **SEARCH)


@functools.lru_cache(maxsize=None)
def oracle_register(which, query, w):
    return ro.register(oracle_submap(which, w), VS, poses(which)[query], scans()["clouds"][query][:, :3], **OPTS)


@functools.lru_cache(maxsize=None)
def oracle_linearize(which, query, w, loss=None):
    return ro.linearize(oracle_submap(which, w), VS, poses(which)[query], scans()["clouds"][query][:, :3], OPTS["max_distance"], loss)


def oracle_accept(which, query, w, start=None, **kw):
    """(accepted, reason, registration) of a candidate by the oracle; start: another start pose than the current one."""
    reg = oracle_register(which, query, w) if start is None else \
        ro.register(oracle_submap(which, w), VS, start, scans()["clouds"][query][:, :3], **OPTS)
    rot, trans = lo.correction(poses(which)[query] if start is None else start, reg["pose"])
    a = dict(ACCEPT)
    a.update(kw)
    ok, why = lo.accept(reg["status"], reg["inliers"], reg["points"], reg["rmse"], rot, trans, **a)
    return ok, why, reg


@functools.lru_cache(maxsize=None)
def laps():
    """[120, 12] poses: three laps of 40 frames around a square of side 10 on a grid of 1 m, the second lap on the very same
    positions as the first (exact ties between submaps), the third 1 m higher."""
    side = np.arange(10)
    ring = np.concatenate([np.c_[side, 0 * side], np.c_[10 + 0 * side, side], np.c_[10 - side, 10 + 0 * side], np.c_[0 * side, 10 - side]])
    P = np.zeros((120, 12))
    P[:, :9] = np.eye(3).reshape(9)
    for lap in range(3):
        P[40 * lap:40 * lap + 40, 9:11] = ring
        P[40 * lap:40 * lap + 40, 11] = 1.0 if lap == 2 else 0.0
    return P


LAPS_CASES = [dict(submap_size=4, min_gap=20, max_per_frame=2, query_stride=1, radius=2.5),
              dict(submap_size=4, min_gap=20, max_per_frame=1, query_stride=3, radius=2.5),
              dict(submap_size=7, min_gap=0, max_per_frame=32, query_stride=1, radius=3.0),
              dict(submap_size=70, min_gap=10, max_per_frame=2, query_stride=1, radius=6.0),      # lanes stride inside a submap
              dict(submap_size=1, min_gap=30, max_per_frame=5, query_stride=7, radius=1.0)]
