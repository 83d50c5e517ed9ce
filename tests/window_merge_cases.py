"""Inputs of the window stage's merge (csrc/window_ba.hip: merge_run) on which the expected anchor clouds are known exactly, and
the replay of the merge from the relative poses a call returned.  Shared by tests/test_window_merge_cases_host.py (the
properties the inputs are built for), tests/test_gpu_window_merge.py, tests/test_gpu_window.py and tests/test_gpu_voxel.py.
TEST INFRASTRUCTURE ONLY: no GPU, no product import.

A case is dict(clouds [n] of [m,3] fp32, poses [n,12] = R row-major | t, window_size, leaf).

LATTICE INPUTS.  Points and translations are multiples of 1/64, rotations are proper signed permutation matrices.  Then
every product and sum of the alignment (:268-279), of the relative poses (:284-299) and of R p + t is exact in double and a
multiple of 1/64 of small magnitude, so exactly representable in fp32: summation order, fused multiply-add and BLAS cannot
matter, and oracle.window_oracle.merge_anchors IS the expected answer, with nothing taken from the product.  What is left
to go wrong is what the tests are after: the leaf key (the float quotient, `loc < 0 -> loc - 1` on a face), the first minimum
of d2 in merged order, the sort on re-packed keys of every width, the window code, the bounds between windows.

KEY WIDTHS.  merge_run sorts on kp.total + cbits bits (csrc/key_pack.h: per axis the bit length of max key - min key; cbits:
the width of the window code, 0 for a run of one window), as uint32 keys up to 32 bits and as uint64 keys above.  Leaf 0.125,
identity rotations, a blob of lattice points and two corner points at (k + 0.25) * leaf, which lie in leaf k for either sign
of k and set the minimum and the maximum key of every axis:
    W32   one window    keys -1024..1023, -1024..1023, -512..511   11 + 11 + 10 = 32
    W33   one window    z up to 512                                 11 + 11 + 11 = 33
    wide  one window    -60000..60000 on every axis                 17 + 17 + 17 = 51
    flat32 one window   x in leaf 0, -600000..600000, -1024..1023    0 + 21 + 11 = 32: the x component is shifted by b[1] + b[2]
                        = 32 bits, the full width of the uint32 sort key (the comment in key_compress)
    J32   two windows   -1024..1023, -512..511, -512..511           11 + 10 + 10 = 31, + 1 bit of window code
    J33   two windows   the keys of W32, over both windows          32, + 1 bit of window code
(the joint pass takes the key range over all its windows: J* put the minimum corner into the first and the maximum corner
into the second window).  tests/test_window_merge_cases_host.py asserts these sums from the oracle's keys.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import colorize_oracle as co
from oracle import window_oracle as wo

f32 = np.float32
Q = 64.0                                    # the lattice: multiples of 1/Q
LATTICE_LEAVES = (0.125, 0.0625, 0.1)
WIDTH_LEAF = 0.125
I12 = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])


@functools.lru_cache(maxsize=None)
def rotations24():
    """The 24 proper (det +1) signed permutation matrices."""
    out = []
    for perm in itertools.permutations(range(3)):
        for sgn in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = sgn[r]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    assert len(out) == 24
    return out


def lattice_points(rng, n, half):
    """[n,3] fp32 multiples of 1/64 in [-half, half]."""
    m = int(round(half * Q))
    return (rng.integers(-m, m + 1, (n, 3)) / Q).astype(f32)


def lattice_poses(rng, n, half=0.5, identity=False):
    """[n,12]: a rotation of rotations24 (or the identity) and a translation of multiples of 1/64 in [-half, half]."""
    m = int(round(half * Q))
    Rs = rotations24()
    out = np.zeros((n, 12))
    for i in range(n):
        R = np.eye(3) if identity else Rs[int(rng.integers(24))]
        out[i] = np.concatenate([R.reshape(-1), rng.integers(-m, m + 1, 3) / Q])
    return out


def exact_rel_poses(poses, window_size):
    """The relative poses to the window's first frame (src/lvba_system.cpp:284-299 with the poses as they are, as merge_only
    takes them): R0^T Rj | R0^T (pj - p0).  Exact on lattice poses, where every sum has one non-zero term per entry."""
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    out = np.zeros_like(poses)
    for j in range(len(poses)):
        a = (j // window_size) * window_size
        R0, p0 = poses[a, :9].reshape(3, 3), poses[a, 9:]
        out[j, :9] = (R0.T @ poses[j, :9].reshape(3, 3)).reshape(-1)
        out[j, 9:] = R0.T @ (poses[j, 9:] - p0)
    return out + 0.0                                                      # (-0.0 -> 0.0)


def merged_clouds(clouds, rel_poses, windows, window_size):
    """Per window that is not skipped (None for a skipped one): its frames' colorize_oracle.world_points at their relative
    poses, concatenated in frame order -- the merged cloud before down_sampling_voxel2."""
    n = len(clouds)
    rel_poses = np.asarray(rel_poses, np.float64).reshape(n, 12)
    out = []
    for wi, start in enumerate(range(0, n, window_size)):
        if windows is not None and windows[wi]["skipped"]:
            out.append(None)
            continue
        end = min(start + window_size, n)
        out.append(np.concatenate([co.world_points(clouds[j], rel_poses[j]) for j in range(start, end)]))
    return out


def replay_anchor_clouds(clouds, rel_poses, windows, window_size, leaf):
    """The merge stage restated from the relative poses a call returned: for every window that is not skipped (`windows`: the
    call's per-window dicts with "skipped", or None: none is) the frames' world_points at rel_poses concatenated in frame
    order, thinned by oracle.window_oracle.down_sampling_voxel2 (leaf < 0.001: as they are).  Returns the anchor clouds in
    anchor order.  pose_apply_f32 and leaf_key_of (csrc/scan_points.h) are compiled without contraction and written from left
    to right, as world_points and down_sampling_voxel2 are: the product's clouds must equal these bit for bit."""
    out = []
    for m in merged_clouds(clouds, rel_poses, windows, window_size):
        if m is None:
            continue
        out.append(m if leaf < 0.001 else m[wo.down_sampling_voxel2(m, leaf)])
    return out


def expected(case, leaf=None):
    """(anchor_poses, anchor_clouds, anchor_index) of a lattice case from oracle.window_oracle.merge_anchors."""
    leaf = case["leaf"] if leaf is None else leaf
    ap, ac = wo.merge_anchors(case["clouds"], case["poses"], case["window_size"], leaf)
    n = len(case["clouds"])
    return ap, ac, (np.arange(n) // case["window_size"]).astype(np.int32)


def to_frame(q, pose):
    """The frame coordinates p of the points q of the pose's parent frame: q = R p + t (exact on the lattice)."""
    return ((np.asarray(q, np.float64) - pose[9:]) @ pose[:9].reshape(3, 3)).astype(f32)


# ---------------------------------------------------------------------------------------------------------- lattice
def lattice_case(leaf=0.125, n_frames=7, n_points=3000, window_size=3, seed=11, n_dup=60):
    """7 frames of 3000 lattice points in +-1 m, translations in +-0.5 m, windows of 3 (the last one is ragged: one frame).
    In every window of more than one frame, n_dup points of its first frame are put again, moved exactly, into its last frame:
    the merged cloud then holds the same fp32 point twice and the leaf must emit it once."""
    rng = np.random.default_rng(seed)
    clouds = [lattice_points(rng, n_points, 1.0) for _ in range(n_frames)]
    poses = lattice_poses(rng, n_frames)
    rel = exact_rel_poses(poses, window_size)
    for a in range(0, n_frames, window_size):
        b = min(a + window_size, n_frames) - 1
        if b > a:
            q = co.world_points(clouds[a][:n_dup], rel[a])                # (rel[a] is the identity)
            clouds[b][-n_dup:] = to_frame(q, rel[b])
    return dict(clouds=clouds, poses=poses, window_size=window_size, leaf=leaf)


def tie_stats(merged, leaf):
    """Of one merged cloud: (leaves whose minimum d2 is attained by more than one point, those of them where the points at the
    minimum differ in their coordinates -- a wrong tie rule shows in the output --, points with a negative coordinate exactly on
    a leaf face: negative, and the float quotient an integer)."""
    k, d2 = co.leaf_keys(merged, leaf)
    order = np.lexsort((d2, k[:, 2], k[:, 1], k[:, 0]))
    ks, ds, ps = k[order], d2[order], np.asarray(merged)[order]
    head = np.ones(len(order), bool)
    head[1:] = np.any(ks[1:] != ks[:-1], axis=1)
    starts = np.nonzero(head)[0]
    ends = np.append(starts[1:], len(order))
    tied = distinct = 0
    for a, b in zip(starts, ends):
        m = int(np.sum(ds[a:b] == ds[a]))
        if m > 1:
            tied += 1
            distinct += bool(np.any(ps[a:a + m] != ps[a]))
    loc = (np.asarray(merged, f32).astype(np.float64) / leaf).astype(f32)
    on_face = (loc < 0) & (loc == np.trunc(loc))
    return tied, distinct, int(np.sum(np.any(on_face, axis=1)))


# -------------------------------------------------------------------------------------------------------- key widths
WIDTHS = {                                # name: (windows, per-axis (min key, max key), key bits, window-code bits)
    "W32": (1, ((-1024, 1023), (-1024, 1023), (-512, 511)), 32, 0),
    "W33": (1, ((-1024, 1023), (-1024, 1023), (-512, 512)), 33, 0),
    "wide": (1, ((-60000, 60000),) * 3, 51, 0),
    "flat32": (1, ((0, 0), (-600000, 600000), (-1024, 1023)), 32, 0),
    "J32": (2, ((-1024, 1023), (-512, 511), (-512, 511)), 31, 1),
    "J33": (2, ((-1024, 1023), (-1024, 1023), (-512, 511)), 32, 1),
}


@functools.lru_cache(maxsize=None)
def width_case(name):
    """See the module docstring.  Two frames per window; the blob is dealt over all frames, the minimum corner is the last
    point of the first window's second frame, the maximum corner the first point of the last window's first frame."""
    n_win, rng_k, _, _ = WIDTHS[name]
    rng = np.random.default_rng(5)
    n = 2 * n_win
    blob = lattice_points(rng, 4000, 0.75)
    for j, (k0, k1) in enumerate(rng_k):
        if k0 == k1:                                                       # this axis takes no key bit: all of it in leaf k0
            blob[:, j] = (k0 * WIDTH_LEAF + rng.integers(1, 8, len(blob)) / Q).astype(f32)
    poses = lattice_poses(rng, n, identity=True)
    rel = exact_rel_poses(poses, 2)
    lo = np.array([[(k[0] + 0.25) * WIDTH_LEAF for k in rng_k]])
    hi = np.array([[(k[1] + 0.25) * WIDTH_LEAF for k in rng_k]])
    parts = np.array_split(blob, n)
    clouds = [to_frame(co.world_points(p, I12), rel[j]) for j, p in enumerate(parts)]   # the blob sits in the anchor frame
    clouds[1] = np.concatenate([clouds[1], to_frame(lo, rel[1])])
    clouds[n - 2] = np.concatenate([to_frame(hi, rel[n - 2]), clouds[n - 2]])
    return dict(clouds=clouds, poses=poses, window_size=2, leaf=WIDTH_LEAF)


def key_widths(case):
    """Per axis the bit length of (max - min) of the oracle's leaf keys over the merged points of ALL windows of the case."""
    rel = exact_rel_poses(case["poses"], case["window_size"])
    m = np.concatenate([c for c in merged_clouds(case["clouds"], rel, None, case["window_size"]) if len(c)])
    k, _ = co.leaf_keys(m, case["leaf"])
    return [int(np.ptp(k[:, j])).bit_length() for j in range(3)]


# ------------------------------------------------------------------------------------------------------------ shapes
def _case(rng, counts, window_size, leaf=0.125, half=1.0):
    return dict(clouds=[lattice_points(rng, c, half) for c in counts], poses=lattice_poses(rng, len(counts)),
                window_size=window_size, leaf=leaf)


@functools.lru_cache(maxsize=None)
def shape_cases():
    """name -> case.  The kernels run 256 threads a block over the points of the run of windows."""
    rng = np.random.default_rng(23)
    out = {}
    for total in (255, 256, 257):                                          # one block, exactly; one point into the next
        out[f"total{total}"] = _case(rng, (100, total - 180, 80), 2, half=0.5)           # two windows: the joint pass
        out[f"total{total}_one_window"] = _case(rng, (100, total - 100), 2, half=0.5)
    out["total1"] = _case(rng, (1,), 2)
    out["last_window_of_one_point"] =_case(rng, (300, 200, 1), 2)             # a last window of one frame, of one point
    out["empty_frame_inside"] = _case(rng, (500, 0, 300, 200), 3)          # ... and a last window of one frame
    out["empty_first_frame"] = _case(rng, (0, 400, 300, 0), 2)
    out["all_empty_window"] = _case(rng, (300, 200, 0, 0, 250), 2)
    out["all_empty_only_window"] = _case(rng, (0, 0), 2)
    # one leaf holds 1000 identical points over two frames, so the leader's run crosses several 256-thread blocks; the leaf's
    # survivor is a closer point that comes LAST in merged order.  Around it a blob.
    c = _case(rng, (700, 700, 400), 3, half=0.5)
    rel = exact_rel_poses(c["poses"], 3)
    same = np.tile(np.array([[5 / 64, 6 / 64, 1 / 64]]), (1000, 1))        # leaf (0,0,0) at 0.125; the centre is 4/64
    c["clouds"][0][-600:] = to_frame(same[:600], rel[0])
    c["clouds"][1][:400] = to_frame(same[600:], rel[1])
    c["clouds"][2][-1] = to_frame(np.array([[4 / 64, 5 / 64, 3 / 64]]), rel[2])[0]
    out["thousand_in_one_leaf"] = c
    # one leaf per point: 900 distinct leaves, every point somewhere inside its own
    keys = rng.permutation(np.arange(-450, 450))[:, None] * np.array([[1, -1, 2]]) + np.array([[0, 3, -7]])
    pts = (keys * 8 + rng.integers(1, 8, (900, 3))) / Q                    # leaf 0.125 = 8/64: offsets 1..7 lie inside leaf `keys`
    c = _case(rng, (300, 300, 300), 2)
    rel = exact_rel_poses(c["poses"], 2)
    c["clouds"] = [to_frame(pts[300 * j:300 * (j + 1)], rel[j]) for j in range(3)]
    out["one_leaf_per_point"] = c
    return out


# ------------------------------------------------------------------------------------------------------------ errors
@functools.lru_cache(maxsize=None)
def error_cases():
    """name -> (case, the window that holds the bad point).  Three windows of two frames at identity rotations; the bad point
    sits in the second frame of window 1.  out_of_range: a coordinate of 2^20 leaves (the keys reach -2^20 .. 2^20 - 1);
    nan: a coordinate is infinite, and 0 * inf of the rotation's zero entries makes the other two NaN."""
    out = {}
    for name, bad in (("out_of_range", [float(1 << 20) * WIDTH_LEAF, 0.25, -0.5]), ("nan", [np.inf, 0.25, -0.5])):
        rng = np.random.default_rng(29)
        c = dict(clouds=[lattice_points(rng, 200, 1.0) for _ in range(6)], poses=lattice_poses(rng, 6, identity=True),
                 window_size=2, leaf=WIDTH_LEAF)
        c["poses"][:, 9:] = 0.0
        c["clouds"][3][57] = np.asarray(bad, f32)
        out[name] = (c, 1)
    return out
