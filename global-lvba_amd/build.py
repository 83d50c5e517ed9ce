"""Build liblvba_hip.so (gfx950) in-tree with hipcc.  No torch, no JIT cache: the .so sits next to
this file so it travels with the repo snapshot to the GPU box."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "liblvba_hip.so")
SOURCES = ["lvba_api.hip", "block_system.hip", "balm_kernels.hip", "ldlt.hip", "visual_api.hip", "visual_kernels.hip",
           "voxelize.hip", "window_ba.hip", "tracks.hip", "pair_lists.hip", "fusion.hip", "bcr.hip", "colorize.hip", "priors.hip", "visual_priors.hip", "prior_tables.hip", "map_quality.hip", "register.hip", "loop_candidates.hip", "place.hip", "closures.hip", "pose_graph.hip", "match.hip", "covis.hip", "track_graph.hip", "verify.hip", "sift.hip", "image_set.hip", "dynamic.hip", "resect.hip", "calib.hip", "photo.hip", "palign.hip", "expo.hip", "undistort.hip"]
HEADERS = ["balm_math.h", "lvba_internal.h", "lvba_common.h", "block_system.h", "visual_math.h", "visual_loss.h", "mempool.h", "voxel_internal.h", "scan_points.h", "segments.h", "image_set.h", "pair_lists.h", "tracks_device.h", "ordering.h", "host_tables.h", "host_arena.h", "fusion_device.h", "ldlt_lookahead.h", "ldlt_schedule.h", "ldlt_layout.h", "ldlt_prepare.h", "ldlt_diag.h", "ldlt_tiles.h", "ldlt_back.h", "ldlt_nd.h", "nd_plan.h", "key_pack.h", "colorize_device.h", "prior_device.h", "visual_prior_device.h", "prior_tables.h", "map_quality_device.h", "voxel_lookup.h", "register_device.h", "loop_device.h", "place_device.h", "closure_device.h", "posegraph_device.h", "lm_rule.h", "match_device.h", "covis_device.h", "track_graph_device.h", "verify_device.h", "sift_device.h", "dynamic_device.h", "resect_device.h", "calib_device.h", "calib_td_device.h", "photo_device.h", "palign_device.h", "expo_device.h", "undistort_device.h", "ransac_device.h", "ransac_batch.h", "wave_ops.h", os.path.join("..", "..", "include", "lvba_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
         "-Wall", "-Wno-unused-result", "-Wno-unused-value"]
# Kernels that take DISCRETE decisions on floating-point values (voxel keys, pixel indices, depth / angle / reprojection
# thresholds, fp32 write-backs, neighbourhood membership: the depth renderer, the colouriser, the track fusion, the triangulation, the anchor
# merge and down-sampling, the map-quality metrics, the registration's inlier gate, the loop-closure candidates' radius gate, the scan descriptors' bins,
# the place search's orderings, the closure consistency's two clauses, the descriptor matcher's epipolar and depth gates, the co-visibility selection's
# in-image and occlusion tests, the two-view verification's pivots, inlier counts and winner and the SIFT extractor's fp32 pyramid, whose blur sums are
# part of its rule, with its extremum, contrast, edge and peak tests, the dynamic-point labels' range-image cells and tolerance comparisons, and the
# camera resectioning's three-point solver, inlier counts and winner, and the extrinsic refinement's cheirality test and pixel gate,
# whose per-record terms are the oracle's bit for bit, and the colour fusion's occlusion test and 1/256-pixel texel weights, and the
# photometric alignment, which samples as the fusion does and whose per-sample terms are the oracle's bit for bit, and the
# exposure estimation, which locates a point as the fusion does and is integer arithmetic from there on, and the undistorted
# images, whose source position decides the texels and the 1/256-pixel weights)
# must round like the reference's plain x86-64 build, expression by expression: no contraction of a*b+c into FMAs there.
# The LM kernels (smooth arithmetic, compared at 1e-8) keep the FMAs.
NO_CONTRACT = {"fusion.hip", "tracks.hip", "window_ba.hip", "colorize.hip", "map_quality.hip", "register.hip", "loop_candidates.hip", "place.hip", "closures.hip", "match.hip", "covis.hip", "verify.hip", "sift.hip", "image_set.hip", "dynamic.hip", "resect.hip", "calib.hip", "photo.hip", "palign.hip", "expo.hip", "undistort.hip"}


def flags_for(src):
    return FLAGS + ["-ffp-contract=off" if src in NO_CONTRACT else "-ffp-contract=fast"]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(CSRC, s.replace(".hip", ".o"))
        cmd = [hipcc(), *flags_for(s), "-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd))
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(o)
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{out}")
        if verbose and out.strip():
            print(out)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-ldl"]
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
