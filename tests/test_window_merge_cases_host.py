"""CPU tests (no GPU) of tests/window_merge_cases.py: the properties the inputs of tests/test_gpu_window_merge.py are built
for are conditions on those inputs, asserted here -- ties and on-face points do occur, every key-width case has exactly the
stated widths, and on lattice inputs the replay of the merge from exact relative poses is oracle.window_oracle.merge_anchors
bit for bit (so that the GPU tests may hold the product to either)."""
import numpy as np
import pytest

import window_merge_cases as wc
from oracle import window_oracle as wo


def _assert_replay_equals_merge_anchors(case, leaf):
    ap, ac, _ = wc.expected(case, leaf)
    rel = wc.exact_rel_poses(case["poses"], case["window_size"])
    rep = wc.replay_anchor_clouds(case["clouds"], rel, None, case["window_size"], leaf)
    assert len(rep) == len(ac) == len(ap) == -(-len(case["clouds"]) // case["window_size"])
    for a, b in zip(rep, ac):
        np.testing.assert_array_equal(a, b)


def test_rotations_are_the_24_proper_signed_permutations():
    Rs = wc.rotations24()
    assert len({tuple(R.reshape(-1)) for R in Rs}) == 24
    for R in Rs:
        assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) > 0.5
        assert np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3))


def test_lattice_case_has_ties_face_points_and_duplicates():
    case = wc.lattice_case(0.125)
    assert [len(c) for c in case["clouds"]] == [3000] * 7 and case["window_size"] == 3
    for c in case["clouds"]:
        assert np.array_equal(c * 64, np.round(c * 64)) and np.abs(c).max() <= 2.0   # (+-1 m; the moved duplicates reach further)
    rel = wc.exact_rel_poses(case["poses"], 3)
    assert np.array_equal(rel * 64, np.round(rel * 64))
    merged = wc.merged_clouds(case["clouds"], rel, None, 3)
    assert [len(m) for m in merged] == [9000, 9000, 3000]
    for m in merged:                                                       # the merged points stay on the lattice
        assert np.array_equal(m * 64, np.round(m * 64))
    tied, distinct, on_face = (sum(v) for v in zip(*(wc.tie_stats(m, 0.125) for m in merged)))
    print(f"lattice case at leaf 0.125: {tied} tied leaves, {distinct} of them between different points, {on_face} negative on-face points")
    assert tied >= 100 and on_face >= 1000
    assert distinct >= 100      # ... and the tie is between points that differ, so that picking the last one changes the cloud
    for m in merged[:2]:        # the first frame's duplicates in the window's last frame: the same fp32 rows, twice
        np.testing.assert_array_equal(m[-60:], m[:60])
    # a tie rule that takes the LAST minimum gives another cloud: the cases can tell the two apart
    m = merged[0]
    keep = wo.down_sampling_voxel2(m, 0.125)
    keep_last = len(m) - 1 - wo.down_sampling_voxel2(m[::-1], 0.125)
    assert not np.array_equal(m[keep], m[keep_last])


@pytest.mark.parametrize("leaf", wc.LATTICE_LEAVES + (0.0,))
def test_lattice_replay_equals_merge_anchors(leaf):
    _assert_replay_equals_merge_anchors(wc.lattice_case(leaf), leaf)


@pytest.mark.parametrize("name", sorted(wc.WIDTHS))
def test_key_width_cases_have_the_stated_widths(name):
    n_win, rng_k, key_bits, code_bits = wc.WIDTHS[name]
    case = wc.width_case(name)
    assert len(case["clouds"]) == 2 * n_win and sum(len(c) for c in case["clouds"]) == 4002
    widths = wc.key_widths(case)
    assert widths == [int(hi - lo).bit_length() for lo, hi in rng_k], widths
    assert sum(widths) == key_bits
    assert code_bits == (n_win - 1).bit_length()                          # no window is skipped: codes 0 .. n_win - 1
    assert {"W32": 32, "W33": 33, "wide": 51, "flat32": 32, "J32": 32, "J33": 33}[name] == key_bits + code_bits
    _assert_replay_equals_merge_anchors(case, case["leaf"])
    if n_win == 2:    # the range is that of BOTH windows: the first holds the minimum corner only, the second the maximum
        rel = wc.exact_rel_poses(case["poses"], 2)
        k = [wc.co.leaf_keys(m, case["leaf"])[0] for m in wc.merged_clouds(case["clouds"], rel, None, 2)]
        lo, hi = np.array(rng_k).T
        assert np.array_equal(k[0].min(0), lo) and np.all(k[0].max(0) < hi)
        assert np.array_equal(k[1].max(0), hi) and np.all(k[1].min(0) > lo)


@pytest.mark.parametrize("name", sorted(wc.shape_cases()))
def test_shape_cases(name):
    case = wc.shape_cases()[name]
    total = sum(len(c) for c in case["clouds"])
    _assert_replay_equals_merge_anchors(case, case["leaf"])
    _, ac, _ = wc.expected(case)
    if name.startswith("total"):
        assert total == int(name[5:].split("_")[0])
    if name == "all_empty_window":
        assert [len(a) > 0 for a in ac] == [True, False, True]
    if name == "thousand_in_one_leaf":
        rel = wc.exact_rel_poses(case["poses"], 3)
        m = wc.merged_clouds(case["clouds"], rel, None, 3)[0]
        same = np.all(m == m[100], axis=1)
        assert np.array_equal(np.nonzero(same)[0], np.arange(100, 1100))   # 1000 identical rows in a row, over 4 blocks of 256
        k, _ = wc.co.leaf_keys(m, 0.125)
        assert np.array_equal(k[100], k[-1]) and not np.array_equal(m[100], m[-1])
        assert any(np.array_equal(r, m[-1]) for r in ac[0])                # the last point of the run is the leaf's survivor
        assert not any(np.array_equal(r, m[100]) for r in ac[0])
    if name == "one_leaf_per_point":
        assert sum(len(a) for a in ac) == total == 900


def test_error_cases_are_outside_the_key_range():
    for name, (case, bad_window) in wc.error_cases().items():
        rel = wc.exact_rel_poses(case["poses"], 2)
        with np.errstate(invalid="ignore"):
            merged = wc.merged_clouds(case["clouds"], rel, None, 2)
        for wi, m in enumerate(merged):
            with np.errstate(invalid="ignore"):
                loc = (m.astype(np.float64) / case["leaf"]).astype(np.float32)
                ok = bool(np.all(np.abs(loc) < 2 ** 20))
            assert ok == (wi != bad_window), (name, wi)
        if name == "nan":
            assert np.isnan(merged[bad_window]).any() and not np.isnan(np.concatenate(case["clouds"])).any()
        else:
            assert merged[bad_window].max() == 2.0 ** 20 * case["leaf"]
