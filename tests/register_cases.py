"""The shared registration fixture of tests/test_register_host.py and tests/test_gpu_register.py, computed once per process.

make_scans(6, 3000, room=(8, 6, 3)): frames 0-4 at their true poses are the map, frame 5 is registered.  The generator's
remaining arguments, the map's eigen ratios, the gate and the start come from the CPU study written up in DESIGN.md §10c
(plain Gauss-Newton walks away from the truth on a map cut with the stage-1 ratios at 15 % clutter):
  seed 5, noise 5 mm, 5 % clutter, eigen ratios 0.02 on every layer, gate 0.1 m, no loss, start 2 degrees / 0.1 m off.
With these the oracle has, as the conditions on the fixture ask,
  at the true pose     1498 inliers of 3000 points, rmse 6.4 mm < 3 x noise
  from the start       converged at the 4th linearisation, 7.1e-4 rad and 0.8 mm from poses_gt
  decision margins     >= 1.6e-6 m on every linearisation (the bar is 1e-9 m)
Seed 3 (the one the other voxel tests use) was tried first and dropped: only 500 of its 3000 query points find a plane and the
fit ends 3.8 mm / 1.1e-3 rad from the truth at best.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np

from oracle import voxel_oracle as vo
import register_oracle as ro

VS = 1.0
RATIO = np.float32([0.02, 0.02, 0.02, 0.02])
GATE = 0.1
NOISE = 0.005
OPTS = dict(max_iterations=30, max_distance=GATE, min_inliers=100, min_eigenvalue=1e-3, tol_rot=1e-6, tol_pos=1e-6)
MAP_FRAMES, QUERY = 5, 5


@functools.lru_cache(maxsize=None)
def scans():
    synth = importlib.import_module("global-lvba_amd.synth")
    return synth.make_scans(6, 3000, room=(8, 6, 3), origin=(2.5, -1.5, 0.2), n_panels=6, seed=5, noise=NOISE, clutter_frac=0.05)


@functools.lru_cache(maxsize=None)
def oracle_map():
    s = scans()
    surf, vox = vo.build([c[:, :3] for c in s["clouds"][:MAP_FRAMES]], s["poses_gt"][:MAP_FRAMES], VS, RATIO)
    return surf


def query_points():
    return scans()["clouds"][QUERY][:, :3]


def truth():
    return scans()["poses_gt"][QUERY].copy()


def start():
    return ro.perturb(truth(), np.radians(2.0), 0.1, 1)


@functools.lru_cache(maxsize=None)
def oracle_linearize(which):
    T = {"truth": truth, "start": start}[which]()
    return ro.linearize(oracle_map(), VS, T, query_points(), GATE)


@functools.lru_cache(maxsize=None)
def oracle_register():
    return ro.register(oracle_map(), VS, start(), query_points(), **OPTS)
