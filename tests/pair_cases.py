"""LiDAR-BA problems with a CHOSEN pair-list geometry, and the item lists the library must build for them.

The pair pass forms every off-diagonal pose block -sum Y_i Y_j^T from a list of pairs.  How those lists are
cut into work items decides which index arithmetic of balm_pair_col_kernel / balm_pair_staged_kernel / balm_pair_reduce_kernel runs;
the synthetic generator never puts a list at a boundary.  Here the voxels are laid out so that it does:

  * a voxel seen by two poses (i, j) adds exactly one pair to exactly one block, so block (i, j) of voxel window w has as many
    pairs as there are {i, j} voxels in window w (plus what larger cliques add);
  * a backbone of three-observer voxels (p, p+1, p+2) keeps the co-visibility graph connected; the designed blocks join poses
    at least three apart, which the backbone never touches.

Every voxel is a plane patch in the world frame whose points are moved into each observing body frame and rounded to fp32 (the
construction of test_voxels_with_more_observers_than_lanes).  Pure numpy: no GPU, no library call.

predict() restates the documented rules of csrc/pair_lists.hip (key = window | tile(J/8, I/8) | J%8 | I%8, stable sort, runs cut
at LVBA_PAIR_CUT and laid out longest first inside a window), csrc/block_system.hip (windows are dropped when a block appears in
more than 24 pieces on average) and csrc/host_tables.h (pair_cut_length, group_pair_items) for problems that keep the caller's pose
order (6 N <= 1024: no ordering is computed).
"""
from __future__ import annotations

import functools
from collections import Counter, namedtuple

import numpy as np

PAIR_CUT = 32          # LVBA_PAIR_CUT (csrc/lvba_internal.h)
PC_ITEMS = 10          # items per wavefront of the column kernel; 4 wavefronts per workgroup
NPTS = 20

Item = namedtuple("Item", "win I J len partial")        # I > J; partial: the item writes a partial block
Case = namedtuple("Case", "name N voxels window backbone")


def pair_cut_length(Q):
    """host_tables.h"""
    return max(64, min((Q // 4096 + 15) // 16 * 16, 512))


# ---------------------------------------------------------------------------------------------------------------------------
# the library's item list, from its documented rules
# ---------------------------------------------------------------------------------------------------------------------------
def _runs(N, voxels, window):
    """(window, I, J) runs in key order with their pair counts; pairs of a run stay in voxel order"""
    tpr = N // 8 + 1
    cnt = Counter()
    for a, obs in enumerate(voxels):
        w = a // window if window > 0 else 0
        for x in range(len(obs)):
            for y in range(x + 1, len(obs)):
                I, J = max(obs[x], obs[y]), min(obs[x], obs[y])
                cnt[(w, (J >> 3) * tpr + (I >> 3), J & 7, I & 7, I, J)] += 1
    return [(k[0], k[4], k[5], cnt[k]) for k in sorted(cnt)]


def predict(N, voxels, window):
    """dict(form, cut, window_voxels, items [Item], n_multi, n_partial, partials {(I, J): count}, longest_item, longest_multi)"""
    assert 6 * N <= 1024, "larger systems are re-ordered: the prediction assumes the caller's pose order"
    Q = sum(len(o) * (len(o) - 1) // 2 for o in voxels)
    pieces, col = None, False
    if window > 0:
        pieces = []
        for w, I, J, n in _runs(N, voxels, window):
            pieces += [(w, I, J, min(PAIR_CUT, n - q)) for q in range(0, n, PAIR_CUT)]
        pieces.sort(key=lambda p: (p[0], -p[3]))                       # stable: equal lengths stay in (tile, block) order
        col = len(pieces) <= 24 * len({(p[1], p[2]) for p in pieces})
    if not col:
        window = 0
        pieces = _runs(N, voxels, 0)
    cut = PAIR_CUT if col else pair_cut_length(Q)
    cutp = []
    for w, I, J, n in pieces:
        cutp += [(w, I, J, min(cut, n - q)) for q in range(0, n, cut)]
    per_block = Counter((I, J) for _, I, J, _ in cutp)
    items = [Item(w, I, J, n, per_block[(I, J)] > 1) for w, I, J, n in cutp]
    partials = {b: c for b, c in per_block.items() if c > 1}
    return dict(form=1 if col else 0, cut=cut, window_voxels=window, items=items, n_multi=len(partials),
                n_partial=sum(partials.values()), partials=partials, longest_item=max(i.len for i in items),
                longest_multi=max(partials.values(), default=0), Q=Q)


# ---------------------------------------------------------------------------------------------------------------------------
# voxel orders
# ---------------------------------------------------------------------------------------------------------------------------
def far_blocks(N):
    """pose pairs (j, i), i >= j + 3: blocks the backbone does not touch"""
    return [(j, i) for j in range(N) for i in range(j + 3, N)]


def backbone(N):
    return [(p, p + 1, p + 2) for p in range(N - 2)]


def lay_out(N, windows, mode):
    """Voxel order of `windows` (each a list of (pose tuple, count)) and the voxels per window.  mode "first": the backbone joins
    window 0 (cases of one window); "pad": windows shorter than the longest are filled with backbone voxels taken in turn, what is
    left of the backbone follows; "tail": the windows all have one length and the backbone follows them; None: no backbone."""
    wins = [[tuple(obs) for obs, n in w for _ in range(n)] for w in windows]
    bb = backbone(N)
    if mode == "first":
        wins[0] += bb
        bb = []
    W = max(len(w) for w in wins)
    if mode == "pad":
        k = 0
        for w in wins:
            while len(w) < W:
                w.append(bb[k % len(bb)])
                k += 1
        bb = bb[k:] if k < len(bb) else []
    if mode in ("pad", "tail") and bb:
        wins += [bb[o:o + W] for o in range(0, len(bb), W)]
    assert all(len(w) == W for w in wins[:-1]), [len(w) for w in wins]
    return [o for w in wins for o in w], W


def _one_window(name, N, groups, mode="first"):
    vox, W = lay_out(N, [groups], mode)
    return Case(name, N, vox, W, mode)


def _item_count_case(name, K):
    """exactly K items in one window under either kernel: the backbone's 2 N - 3 blocks plus two-observer voxels on far blocks"""
    if K == 1:
        return Case(name, 2, [(0, 1)], 1, None)
    N = next(n for n in range(3, 49) if 2 * n - 3 <= K <= 2 * n - 3 + len(far_blocks(n)))
    return _one_window(name, N, [(b, 1 + e % 4) for e, b in enumerate(far_blocks(N)[:K - (2 * N - 3)])])


LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 96]
REDUCER = [2, 3, 4, 5, 7, 8, 9]
# The mixed-wavefront case: windows of three items each (lengths longest first inside a window only), so a wavefront's ten items
# span four windows and are not monotone.  Wavefront f has ONE longest item (32 pairs, the others at most 30), and it sits at item
# MIXED_MAX_AT[f] of the ten: every position once, so the wavefront's round count must come from a maximum over all ten.
MIXED_MAX_AT = [9, 8, 7, 0, 2, 1, 3, 5, 4, 6]
_MIXED_PLAIN = [(20, 17, 1), (30, 7, 1), (17, 16, 5), (13, 13, 12), (19, 18, 1), (25, 12, 1), (28, 5, 5)]


def _mixed():
    assert all((PC_ITEMS * f + p) % 3 == 0 for f, p in enumerate(MIXED_MAX_AT))      # a window's first item
    special = {(PC_ITEMS * f + p) // 3 for f, p in enumerate(MIXED_MAX_AT)}
    return [((32, 5, 1) if w % 2 else (32, 3, 3)) if w in special else _MIXED_PLAIN[w % 7] for w in range(34)]


MIXED = _mixed()
LANE_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 129]
COL_ITEM_COUNTS = [1, 9, 10, 11, 39, 40, 41, 319, 320, 321]
LANE_ITEM_COUNTS = [1, 15, 16, 17, 127, 128, 129]


def lengths_blocks():
    return far_blocks(12)[::4][:len(LENGTHS)]


def reducer_blocks():
    return far_blocks(12)[1::5][:len(REDUCER)]


def lane_lengths_blocks():
    return far_blocks(12)[2::4][:len(LANE_LENGTHS)]


def _cases():
    c = {}
    c["lengths"] = _one_window("lengths", 12, list(zip(lengths_blocks(), LENGTHS)))
    # block k of the reducer case is seen in the first REDUCER[k] windows (1 .. 3 pairs there): that many partial blocks
    wins = [[(b, 1 + (w + k) % 3) for k, (b, n) in enumerate(zip(reducer_blocks(), REDUCER)) if w < n] for w in range(max(REDUCER))]
    vox, W = lay_out(12, wins, "pad")
    c["reducer"] = Case("reducer", 12, vox, W, "pad")
    for K in COL_ITEM_COUNTS:
        c[f"items_{K}"] = _item_count_case(f"items_{K}", K)
    pool = far_blocks(10)[::3][:7]
    wins = [[(pool[(3 * w + r) % 7], n) for r, n in enumerate(t)] for w, t in enumerate(MIXED)]
    vox, W = lay_out(10, wins, "tail")
    c["mixed"] = Case("mixed", 10, vox, W, "tail")
    c["short_array"] = _one_window("short_array", 4, [((0, 3), 5)])
    fb = far_blocks(8)
    vox, W = lay_out(8, [[(fb[0], 32), (fb[5], 4)], [], [(fb[9], 35), (fb[12], 1)]], "pad")
    c["ends"] = Case("ends", 8, vox, W, "pad")
    for N in (7, 8, 9):
        c[f"tiles_{N}"] = _one_window(f"tiles_{N}", N, [((j, i), 1 + (3 * i + j) % 4) for j, i in far_blocks(N)])
    c["fallback"] = Case("fallback", 4, [(0, 1, 2, 3)] * 200, 4, None)
    # 16-lane kernel only (no windows)
    c["lane_lengths"] = _one_window("lane_lengths", 12, list(zip(lane_lengths_blocks(), LANE_LENGTHS)))._replace(window=0)
    for K in LANE_ITEM_COUNTS:
        c[f"lane_items_{K}"] = _item_count_case(f"lane_items_{K}", K)._replace(window=0)
    c["lane_window_stage"] = Case("lane_window_stage", 20, [tuple(range(20))] * 1400, 0, None)
    c["lane_long_cut"] = Case("lane_long_cut", 21, [tuple(range(21))] * 1280, 0, None)   # Q = 268 800: pair_cut_length 80
    return c


CASES = _cases()
COL_CASES = [n for n, c in CASES.items() if c.window > 0]
LANE_CASES = [n for n, c in CASES.items() if c.window == 0]
Y32_CASES = ["lengths", "reducer", "mixed"]


@functools.lru_cache(maxsize=None)
def prediction(name, window=None):
    c = CASES[name]
    return predict(c.N, c.voxels, c.window if window is None else window)


# ---------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------
def _exp_so3(w):
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    th2 = np.maximum(th, 1e-12)
    return np.eye(3) + np.sin(th2) / th2 * K + (1 - np.cos(th2)) / th2 ** 2 * (K @ K)


def _pack(R, t):
    return np.concatenate([R.reshape(-1, 9), t], axis=1)


def arrays(N, voxels, seed):
    """dict(n_poses, voxel_off, pose_idx, clusters, poses_gt, poses_init) of the voxels (pose tuples) in the given order"""
    rng = np.random.default_rng(seed)
    R = _exp_so3(rng.uniform(-0.3, 0.3, (N, 3)))
    t = rng.uniform([0.0, 0.0, 0.0], [4.0, 4.0, 1.0], (N, 3))
    R0 = R @ _exp_so3(rng.normal(0.0, np.radians(0.02), (N, 3)))
    t0 = t + rng.normal(0.0, 0.01, (N, 3))
    V = len(voxels)
    k = np.array([len(o) for o in voxels])
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    idx = np.concatenate([np.asarray(o) for o in voxels]).astype(np.int32)
    vox = np.repeat(np.arange(V), k)
    n = rng.normal(size=(V, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    e1 = np.cross(n, np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(n, e1)
    c = rng.uniform([-3.0, -3.0, -2.0], [7.0, 7.0, 3.0], (V, 3))
    F = len(idx)
    ab = rng.uniform(-0.4, 0.4, (F, NPTS, 2))                              # every observer samples the patch anew
    h = rng.normal(0.0, 0.01, (F, NPTS))
    pw = c[vox, None, :] + ab[..., :1] * e1[vox, None, :] + ab[..., 1:] * e2[vox, None, :] + h[..., None] * n[vox, None, :]
    pb = np.einsum("fpi,fij->fpj", pw - t[idx][:, None, :], R[idx]).astype(np.float32).astype(np.float64)
    x, y, z = pb[..., 0], pb[..., 1], pb[..., 2]
    clu = np.stack([(x * x).sum(1), (x * y).sum(1), (x * z).sum(1), (y * y).sum(1), (y * z).sum(1), (z * z).sum(1),
                    x.sum(1), y.sum(1), z.sum(1), np.full(F, float(NPTS))], axis=1)
    return dict(n_poses=N, voxel_off=off, pose_idx=idx, clusters=clu, poses_gt=_pack(R, t), poses_init=_pack(R0, t0))


@functools.lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    d = arrays(c.N, c.voxels, 1000 + sorted(CASES).index(name))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def without_voxel(d, v):
    """the problem with voxel v left out"""
    off = d["voxel_off"]
    keep = np.ones(off[-1], bool)
    keep[off[v]:off[v + 1]] = False
    k = np.delete(np.diff(off), v)
    return dict(d, voxel_off=np.concatenate([[0], np.cumsum(k)]).astype(np.int64), pose_idx=d["pose_idx"][keep],
                clusters=d["clusters"][keep])


def feeders(name):
    """{(I, J): [(window, voxel), ...]} in voxel order: the voxels that add a pair to each block, by the case's own windows"""
    c = CASES[name]
    out = {}
    for a, obs in enumerate(c.voxels):
        for x in range(len(obs)):
            for y in range(x + 1, len(obs)):
                out.setdefault((max(obs[x], obs[y]), min(obs[x], obs[y])), []).append((a // c.window if c.window > 0 else 0, a))
    return out


def voxels_to_probe(name):
    """The voxels the sensitivity condition leaves out: every voxel of a block's list, or for lists of more than 64 pairs one in
    eight plus the first and last voxel of every item of the block."""
    p = prediction(name)
    pick = set()
    for (I, J), lst in feeders(name).items():
        if len(lst) <= 64:
            pick.update(a for _, a in lst)
            continue
        pick.update(a for _, a in lst[::8])
        by_win = {}
        for w, a in lst:
            by_win.setdefault(w if p["window_voxels"] else 0, []).append(a)
        for vs in by_win.values():
            for q in range(0, len(vs), p["cut"]):
                pick.update((vs[q], vs[min(q + p["cut"], len(vs)) - 1]))
    return sorted(pick)
