"""CPU tests of the tile-list arithmetic the batched RANSAC stages share (csrc/ransac_device.h, DESIGN.md §10k "The skeleton"):
which tasks get hypothesis blocks, where their block records start, the (task, first hypothesis) list that is the hypothesis
kernel's grid, and the refusal above 2^30 - 1 blocks, which is decided in 64 bits before anything is built."""
import ctypes
import time

import numpy as np
import pytest

from host_build import build_check

HB = 64                       # RANSAC_HB
MAX_BLOCKS = 2 ** 30 - 1      # RANSAC_MAX_BLOCKS = INT32_MAX / 2, the bound the two stages had
INT32_MAX = 2 ** 31 - 1
UNTOUCHED = -7


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/ransac_device.h compiled for the host (tests/ransac_check.cpp)"""
    lib = ctypes.CDLL(build_check("ransac_check", tmp_path_factory.mktemp("emul_ransac")))
    P, I, L = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.emul_plan.argtypes = [L, P, I, I, I, I, P, P, L, P, P]
    lib.emul_plan.restype = L
    return lib


def plan(emul, m, H, need, hb=HB, build=True, cap=None):
    """(n, blk0, n_blk, tiles, last) of ransac_plan, with the list (build) or the count alone"""
    m = np.ascontiguousarray(m, np.int32)
    blk0, n_blk = np.full(len(m), UNTOUCHED, np.int32), np.full(len(m), UNTOUCHED, np.int32)
    cap = (len(m) * -(-H // hb) if cap is None else cap) if build else 0
    tiles, last = np.full((cap, 2), UNTOUCHED, np.int32), np.full(2, UNTOUCHED, np.int32)
    n = emul.emul_plan(len(m), m.ctypes.data, H, hb, need, int(build), blk0.ctypes.data, n_blk.ctypes.data, cap, tiles.ctypes.data, last.ctypes.data)
    return n, blk0, n_blk, tiles[:max(min(n, cap), 0)], last


def want(m, H, need, hb=HB):
    """the rule restated: ceil(H / hb) blocks for a task with m >= need, in task order"""
    per = -(-H // hb)
    n_blk = np.where(np.asarray(m) >= need, per, 0)
    blk0 = np.concatenate([[0], np.cumsum(n_blk)[:-1]]) if len(n_blk) else np.zeros(0, np.int64)
    tiles = [(p, k * hb) for p in range(len(n_blk)) for k in range(n_blk[p])]
    return int(n_blk.sum()), blk0, n_blk, np.array(tiles, np.int64).reshape(-1, 2)


def check(emul, m, H, need, hb=HB):
    n, blk0, n_blk, tiles, last = plan(emul, m, H, need, hb)
    wn, wblk0, wn_blk, wtiles = want(m, H, need, hb)
    assert n == wn
    np.testing.assert_array_equal(blk0, wblk0); np.testing.assert_array_equal(n_blk, wn_blk); np.testing.assert_array_equal(tiles, wtiles)
    if n:
        assert tuple(last) == tuple(wtiles[-1])
    # every tile is where its task's block record is, and a task's tiles cover [0, H) without a gap
    for p in range(len(m)):
        mine = tiles[blk0[p]:blk0[p] + n_blk[p]]
        assert (mine[:, 0] == p).all()
        if n_blk[p]:
            np.testing.assert_array_equal(mine[:, 1], np.arange(n_blk[p]) * hb)
            assert mine[-1, 1] < H <= mine[-1, 1] + hb
    assert plan(emul, m, H, need, hb, build=False)[0] == wn                      # the count alone says the same
    return n, blk0, n_blk, tiles


def test_tile_list_small_cases(emul):
    for H in (1, 63, 64, 65, 200, 1024):
        # no task; every task below the threshold; one task; a batch with refused tasks at the start, in the middle, in a row, at the end
        n, _, _, tiles = check(emul, [], H, 8)
        assert n == 0 and len(tiles) == 0
        n, blk0, n_blk, _ = check(emul, [0, 7, 3], H, 8)
        assert n == 0 and not blk0.any() and not n_blk.any()
        n, _, n_blk, _ = check(emul, [8], H, 8)
        assert n == -(-H // HB) == {1: 1, 63: 1, 64: 1, 65: 2, 200: 4, 1024: 16}[H]
        n, blk0, n_blk, _ = check(emul, [40, 7, 40], H, 8)
        assert n_blk[1] == 0 and blk0[1] == blk0[2] == n_blk[0] and n == 2 * n_blk[0]   # the neighbours' records stay contiguous
        check(emul, [3, 100, 8, 7, 0, 64, 65, 2, 1025, 7], H, 8)
    # the threshold: the diagnostic call asks for k, the others for max(k, min_inliers)
    for k, min_inliers in ((8, 15), (2, 15), (4, 30), (8, 0), (4, 3)):
        m = [k - 1, k, max(k, min_inliers) - 1, max(k, min_inliers), 1000]
        _, _, n_blk, _ = check(emul, m, 65, k)
        np.testing.assert_array_equal(n_blk > 0, np.array(m) >= k)
        _, _, n_blk, _ = check(emul, m, 65, max(k, min_inliers))
        np.testing.assert_array_equal(n_blk > 0, np.array(m) >= max(k, min_inliers))
    check(emul, [5, 9, 5], 10, 5, hb=1)
    check(emul, [5, 9, 5], 10, 5, hb=3)


def test_block_count_is_decided_in_64_bits_before_anything_is_built(emul):
    """The refusals allocate nothing and leave the tasks as they were; each is decided in well under a second (milliseconds: the
    time is printed).  With RANSAC_HB = 64 no H of one or two tasks reaches the bound -- H = INT32_MAX is 2^25 blocks a task, and
    two tasks' 2^26 are accepted like H = INT32_MAX - 63 before them, where the old loop's `int h0 += 64` did not yet overflow --
    so the refusal at H = INT32_MAX with two eligible tasks is shown where it is one under the stated bound, at block widths 1 and
    2 (2^32 and 2^31 blocks), and at width 64 the same call is held to its exact count."""
    t0 = time.perf_counter()
    for hb in (1, 2):
        n, blk0, n_blk, tiles, last = plan(emul, [100, 100], INT32_MAX, 8, hb=hb, cap=4)
        assert n == -1 and (blk0 == UNTOUCHED).all() and (n_blk == UNTOUCHED).all() and len(tiles) == 0 and (last == UNTOUCHED).all()
    n, blk0, n_blk, _, _ = plan(emul, [100, 100], INT32_MAX, 8, build=False)
    assert n == 2 ** 26 and blk0.tolist() == [0, 2 ** 25] and n_blk.tolist() == [2 ** 25, 2 ** 25]
    # one refused task between them changes nothing; three tasks at width 1 overflow 32 bits twice over
    n, blk0, n_blk, _, _ = plan(emul, [100, 7, 100], INT32_MAX, 8, build=False)
    assert n == 2 ** 26 and blk0.tolist() == [0, 2 ** 25, 2 ** 25] and n_blk.tolist() == [2 ** 25, 0, 2 ** 25]
    assert plan(emul, [100, 100, 100], INT32_MAX, 8, hb=1, cap=4)[0] == -1
    # task count x block count either side of the bound: 2^30 - 1 = 32767 x 32769
    m = np.full(32769, 50, np.int32)
    assert MAX_BLOCKS == 32767 * 32769
    n, blk0, n_blk, _, _ = plan(emul, m, 32767 * HB, 8, build=False)
    assert n == MAX_BLOCKS and (n_blk == 32767).all() and blk0[-1] == MAX_BLOCKS - 32767
    n, blk0, n_blk, tiles, _ = plan(emul, m, 32767 * HB + 1, 8, cap=4)                       # 32768 blocks a task: 2^30 + 32768
    assert n == -1 and (blk0 == UNTOUCHED).all() and (n_blk == UNTOUCHED).all() and len(tiles) == 0
    m = np.full(2 ** 20 + 1, 50, np.int32)
    assert plan(emul, m, 1024 * HB, 8, cap=4)[0] == -1                                       # 2^30 + 1024
    m[5] = 7                                                                                 # one task fewer is eligible: 2^30 exactly
    assert plan(emul, m, 1024 * HB, 8, cap=4)[0] == -1
    m[6] = 7
    assert plan(emul, m, 1024 * HB, 8, build=False)[0] == 2 ** 30 - 1024
    dt = time.perf_counter() - t0
    print("refusals and counts decided in %.1f ms" % (1e3 * dt))
    assert dt < 1.0


def test_largest_hypothesis_count_of_one_task(emul):
    """H = INT32_MAX, the largest check_opts lets through, for one task: ceil(H / 64) = 2^25 blocks, the counter never above
    H - 1, the last tile reaching the last hypothesis."""
    n, blk0, n_blk, tiles, last = plan(emul, [100], INT32_MAX, 8, cap=3)
    assert n == -(-INT32_MAX // HB) == 2 ** 25 and blk0[0] == 0 and n_blk[0] == n
    np.testing.assert_array_equal(tiles, [(0, 0), (0, 64), (0, 128)])
    assert last[0] == 0 and last[1] == (n - 1) * HB and last[1] <= INT32_MAX - 1 <= last[1] + 63
