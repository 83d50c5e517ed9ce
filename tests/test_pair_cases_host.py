"""CPU conditions on the problems of tests/pair_cases.py, checked from the oracle alone -- so that tests/test_gpu_pair_pass.py
cannot pass vacuously: every case's predicted item list holds the edge the case is named for; no oracle block lies under
oracle.block_parity's absolute floor (1e-6 of the largest block), where a per-block relative error stops being relative; and
every pair matters -- leaving one voxel out moves every block it feeds by at least 100 x the GPU bar of 1e-8, relative to the
block's largest entry, so a dropped or doubled pair cannot hide under the bar."""
from collections import Counter

import numpy as np
import pytest

import pair_cases as pc

GPU_BAR = 1e-8
SENSITIVITY = 100 * GPU_BAR


def _lens(p, block):
    I, J = max(block), min(block)
    return [i.len for i in p["items"] if (i.I, i.J) == (I, J)]


def _wavefront_nit(n_items):
    return n_items - (n_items - 1) // pc.PC_ITEMS * pc.PC_ITEMS


def test_lengths_case_cuts_at_32():
    p = pc.prediction("lengths")
    assert (p["form"], p["cut"], p["window_voxels"]) == (1, 32, len(pc.CASES["lengths"].voxels))
    want = {1: [1], 2: [2], 31: [31], 32: [32], 33: [32, 1], 63: [32, 31], 64: [32, 32], 65: [32, 32, 1], 96: [32, 32, 32]}
    for b, n in zip(pc.lengths_blocks(), pc.LENGTHS):
        assert _lens(p, b) == want[n], (b, n)
        assert p["partials"].get((b[1], b[0]), 1) == len(want[n])
    assert p["longest_item"] == 32 and p["n_multi"] == 5 and p["n_partial"] == 2 + 2 + 2 + 3 + 3
    # one window: the items come longest first
    assert [i.len for i in p["items"]] == sorted((i.len for i in p["items"]), reverse=True)


def test_reducer_case_reaches_the_unrolled_loop_and_every_tail():
    p = pc.prediction("reducer")
    assert p["form"] == 1
    for b, n in zip(pc.reducer_blocks(), pc.REDUCER):
        assert p["partials"][(b[1], b[0])] == n and len({i.win for i in p["items"] if (i.I, i.J) == (b[1], b[0])}) == n
    counts = set(p["partials"].values())
    assert {2, 3, 4, 5, 7, 8, 9} <= counts and {c % 4 for c in counts} == {0, 1, 2, 3}
    assert p["longest_multi"] == 9


@pytest.mark.parametrize("K", pc.COL_ITEM_COUNTS)
def test_column_item_counts(K):
    c, p = pc.CASES[f"items_{K}"], pc.prediction(f"items_{K}")
    assert p["form"] == 1 and len(p["items"]) == K and c.N <= 48
    assert _wavefront_nit(K) == {1: 1, 9: 9, 10: 10, 11: 1, 39: 9, 40: 10, 41: 1, 319: 9, 320: 10, 321: 1}[K]
    wgs = -(-K // (4 * pc.PC_ITEMS))
    assert wgs == {1: 1, 9: 1, 10: 1, 11: 1, 39: 1, 40: 1, 41: 2, 319: 8, 320: 8, 321: 9}[K]      # 9 -> a grid of 16: two per XCD slot
    # the same problem has K items under the 16-lane kernel too
    assert len(pc.prediction(f"items_{K}", 0)["items"]) == K


def test_mixed_wavefront_spans_four_windows():
    p = pc.prediction("mixed")
    first = p["items"][:pc.PC_ITEMS]
    assert [i.len for i in first] == [20, 17, 1, 30, 7, 1, 17, 16, 5, 32]
    assert [i.win for i in first] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert [tuple(i.len for i in p["items"][3 * w:3 * w + 3]) for w in range(len(pc.MIXED))] == pc.MIXED
    assert max(i.len for i in first) == 32 * min(i.len for i in first)
    # every wavefront has one longest item, and over the wavefronts it sits at each of the ten positions once: a round count taken
    # from fewer than ten lanes drops pairs in this case
    at = []
    for f in range(len(pc.MIXED_MAX_AT)):
        lens = [i.len for i in p["items"][pc.PC_ITEMS * f:pc.PC_ITEMS * (f + 1)]]
        assert len(lens) == 10 and len({i.win for i in p["items"][pc.PC_ITEMS * f:pc.PC_ITEMS * (f + 1)]}) >= 4
        assert lens.count(32) == 1 and sorted(lens)[-2] <= 30 and lens != sorted(lens, reverse=True)
        at.append(lens.index(32))
    assert at == pc.MIXED_MAX_AT and sorted(at) == list(range(10))
    assert p["n_multi"] == 7 and sorted(p["partials"].values()) == [14, 14, 14, 15, 15, 15, 15] and p["longest_multi"] == 15


def test_array_end_cases():
    p = pc.prediction("short_array")
    assert p["form"] == 1 and p["Q"] == 11 < 64
    p = pc.prediction("ends")
    assert p["form"] == 1 and p["items"][0].len == 32 and p["items"][-1].len == 1
    assert p["items"][-1].win == p["items"][-2].win == 2 and p["items"][-3].len == 32


@pytest.mark.parametrize("N", [7, 8, 9])
def test_tile_key_cases(N):
    c, p = pc.CASES[f"tiles_{N}"], pc.prediction(f"tiles_{N}")
    assert c.N == N and p["form"] == 1
    assert len({(i.I, i.J) for i in p["items"]}) == N * (N - 1) // 2                  # every pose pair is a block
    assert max(i.I for i in p["items"]) >> 3 == (1 if N == 9 else 0) and N // 8 + 1 == (1 if N == 7 else 2)
    # the 16-lane order is the (tile, J % 8, I % 8) key order
    tpr = N // 8 + 1
    keys = [((i.J >> 3) * tpr + (i.I >> 3), i.J & 7, i.I & 7) for i in pc.prediction(f"tiles_{N}", 0)["items"]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_fallback_case_drops_the_windows():
    c, p = pc.CASES["fallback"], pc.prediction("fallback")
    runs = pc._runs(c.N, c.voxels, c.window)
    assert len(runs) == 300 and len({(I, J) for _, I, J, _ in runs}) == 6 and 300 > 24 * 6
    assert (p["form"], p["cut"], p["window_voxels"], len(p["items"])) == (0, 64, 0, 24)
    assert [i.len for i in p["items"]] == [64, 64, 64, 8] * 6 and p["partials"] == {b: 4 for b in p["partials"]} and p["n_multi"] == 6


def test_lane_cases():
    p = pc.prediction("lane_lengths")
    assert (p["form"], p["cut"]) == (0, 64)
    want = {1: [1], 15: [15], 16: [16], 17: [17], 63: [63], 64: [64], 65: [64, 1], 129: [64, 64, 1]}
    for b, n in zip(pc.lane_lengths_blocks(), pc.LANE_LENGTHS):
        assert _lens(p, b) == want[n]
    for K in pc.LANE_ITEM_COUNTS:
        p = pc.prediction(f"lane_items_{K}")
        assert p["form"] == 0 and len(p["items"]) == K
        assert (16 * -(-K // 16) - K) == {1: 15, 15: 1, 16: 0, 17: 15, 127: 1, 128: 0, 129: 15}[K]          # dead groups of the last workgroup
    # the window-stage shape: 20 poses x 1 400 voxels, Q = 266 000.  host_tables.h: (266 000 / 4096 + 15) / 16 * 16 = 64 in integer
    # arithmetic -- the cut only grows from Q = 65 * 4096 on, which lane_long_cut (21 x 1 280: Q = 268 800, 26 880 factors) reaches
    p = pc.prediction("lane_window_stage")
    assert p["Q"] == 266_000 and pc.pair_cut_length(p["Q"]) == 64 and p["cut"] == 64
    assert Counter((i.I, i.J) for i in p["items"]) == {(i, j): 22 for j in range(20) for i in range(j + 1, 20)}
    assert [i.len for i in p["items"][:22]] == [64] * 21 + [56] and sum(len(v) for v in pc.CASES["lane_window_stage"].voxels) == 28_000
    p = pc.prediction("lane_long_cut")
    assert p["Q"] == 268_800 and p["cut"] == 80 and [i.len for i in p["items"][:16]] == [80] * 16
    assert sum(len(v) for v in pc.CASES["lane_long_cut"].voxels) <= 28_000


def test_every_case_keeps_the_callers_order_and_a_connected_graph():
    for name, c in pc.CASES.items():
        assert 6 * c.N <= 1024 and all(len(o) >= 2 and list(o) == sorted(set(o)) and o[-1] < c.N for o in c.voxels), name
        seen, todo = {0}, [0]
        adj = {}
        for o in c.voxels:
            for a in o:
                adj.setdefault(a, set()).update(o)
        while todo:
            for b in adj.get(todo.pop(), ()):
                if b not in seen:
                    seen.add(b)
                    todo.append(b)
        assert len(seen) == c.N, name


def _blocks(oracle_mod, d):
    co = oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"])
    bi, bj, blocks, _, _ = co.eval_sparse(d["poses_init"])
    return {(max(a, b), min(a, b)): blk for a, b, blk in zip(bi.tolist(), bj.tolist(), blocks)}


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_no_block_under_the_floor_and_every_pair_matters(oracle_mod, name):
    d = pc.problem(name)
    full = _blocks(oracle_mod, d)
    scale = {b: np.abs(v).max() for b, v in full.items()}
    assert min(scale.values()) >= 1e-6 * max(scale.values()), name                  # block_parity's floor
    c = pc.CASES[name]
    assert {b for b in full if b[0] != b[1]} == set(pc.feeders(name))
    worst = np.inf
    for v in pc.voxels_to_probe(name):
        part = _blocks(oracle_mod, pc.without_voxel(d, v))
        obs = c.voxels[v]
        for x in range(len(obs)):
            for y in range(x + 1, len(obs)):
                b = (obs[y], obs[x])
                moved = np.abs(full[b] - part.get(b, 0.0)).max() / scale[b]
                worst = min(worst, moved)
                assert moved >= SENSITIVITY, (name, v, b, moved)
    print(f"{name}: smallest block {min(scale.values()) / max(scale.values()):.2e} of the largest; a voxel moves its blocks by >= {worst:.2e}")
