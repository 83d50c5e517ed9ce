"""GPU tests of the window stage's merge (csrc/window_ba.hip: merge_run -- wba_merge_kernel, the sort on re-packed keys,
wba_pick_kernel, the scan and the compaction) against oracle.window_oracle.merge_anchors, POINT FOR POINT: same length, same
fp32 rows, same order.  The inputs come from tests/window_merge_cases.py: all their arithmetic is exact, so the oracle is
the expected answer with nothing taken from the product, and tests/test_window_merge_cases_host.py asserts that they have
the properties they are built for (ties between different points, negative coordinates on leaf faces, sort keys of 32, 33
and 51 bits, with and without the window code).  All calls use merge_only: no LM runs."""
import numpy as np
import pytest

import window_merge_cases as wc

pytestmark = pytest.mark.gpu


def _run(pkg, case, leaf=None):
    """merge_only call -> (the call's dict, the anchor clouds)."""
    leaf = case["leaf"] if leaf is None else leaf
    with pkg.Scans(case["clouds"]) as scans:
        got = scans.window_ba(case["poses"], window_size=case["window_size"], anchor_leaf=leaf, merge_only=True)
    asc = got["anchor_scans"]
    try:
        clouds = [asc.download(a) for a in range(asc.n_frames)]
    finally:
        asc.close()
    return got, clouds


def _assert_equals_oracle(pkg, case, leaf=None):
    leaf = case["leaf"] if leaf is None else leaf
    ap, ac, ai = wc.expected(case, leaf)
    got, clouds = _run(pkg, case, leaf)
    np.testing.assert_array_equal(got["anchor_poses"], ap)
    np.testing.assert_array_equal(got["anchor_index"], ai)
    assert [w["skipped"] for w in got["windows"]] == [0] * len(ac)
    assert [w["anchor"] for w in got["windows"]] == list(range(len(ac)))
    assert [w["n_anchor_points"] for w in got["windows"]] == [len(a) for a in ac]
    np.testing.assert_array_equal(got["rel_poses"], wc.exact_rel_poses(case["poses"], case["window_size"]))
    assert len(clouds) == len(ac)
    for a, (g, w) in enumerate(zip(clouds, ac)):
        np.testing.assert_array_equal(g, w, err_msg=f"anchor {a}")
    return got, clouds


@pytest.mark.parametrize("leaf", wc.LATTICE_LEAVES + (0.0,))
def test_lattice_clouds_equal_the_oracle_point_for_point(pkg, leaf):
    """Three windows (3 + 3 + 1 frames) in one joint pass.  At leaf 0.125 hundreds of leaves hold several different points at
    the same minimum d2 (the first in merged order survives) and thousands of points have a negative coordinate exactly on a
    leaf face (they belong one leaf lower: `loc < 0 -> loc - 1` in float); leaf 0.1 is no power of two, so the quotient is
    rounded; leaf 0: no thinning, the merged points as they are."""
    _assert_equals_oracle(pkg, wc.lattice_case(leaf), leaf)


@pytest.mark.parametrize("name", sorted(wc.WIDTHS))
def test_every_sort_key_width_gives_the_oracle_clouds(pkg, name):
    """W32 / J32: exactly 32 sort bits, still uint32 keys; flat32: the same with no bit for x, whose (zero) component is shifted
    by b[1] + b[2] = 32, the key's full width (csrc/key_pack.h); W33 / J33: one bit more, the first uint64 keys, compressed in
    place; wide: 51 bits.  J*: the window code above the key bits, the key range taken over both windows."""
    case = wc.width_case(name)
    _assert_equals_oracle(pkg, case)
    _assert_equals_oracle(pkg, case, 0.0)


@pytest.mark.parametrize("name", sorted(set(wc.shape_cases()) - {"all_empty_window", "all_empty_only_window"}))
def test_shape_edges_give_the_oracle_clouds(pkg, name):
    case = wc.shape_cases()[name]
    _assert_equals_oracle(pkg, case)
    _assert_equals_oracle(pkg, case, 0.0)


@pytest.mark.parametrize("name", ["all_empty_window", "all_empty_only_window"])
def test_a_window_without_points_is_an_anchor_with_an_empty_cloud(pkg, name):
    """DECISION: the product is right to do what the oracle does.  optimizeCameraPoses (src/lvba_system.cpp:1466-1489) walks the
    windows by frame count alone: it pushes the first frame's pose and the merged, thinned cloud of every window, whatever the
    cloud holds -- nothing there skips a window for being empty (the skip rule of runWindowBA, :258-262, counts plane voxels and
    does not exist with merge_only).  So a window whose frames are all empty yields an anchor pose with an empty cloud, the
    anchors after it keep their numbers, and anchor_index stays frame // window_size."""
    case = wc.shape_cases()[name]
    for leaf in (case["leaf"], 0.0):
        got, clouds = _assert_equals_oracle(pkg, case, leaf)
        empty = [sum(len(c) for c in case["clouds"][s:s + 2]) == 0 for s in range(0, len(case["clouds"]), 2)]
        assert [len(c) == 0 for c in clouds] == empty and any(empty)


@pytest.mark.parametrize("name", sorted(wc.error_cases()))
def test_a_point_outside_the_leaf_range_is_refused_and_names_its_window(pkg, name):
    """A merged point at 2^20 leaves, or NaN after the transform: LVBA_ERR_ARG, the message names the window (the joint pass
    fails first and the windows are then run one by one); without thinning there are no keys and the call succeeds; a good
    call afterwards is unaffected."""
    L = pkg._lib
    case, bad_window = wc.error_cases()[name]
    with pkg.Scans(case["clouds"]) as scans:
        with pytest.raises(L.LvbaError) as e:
            scans.window_ba(case["poses"], window_size=2, anchor_leaf=case["leaf"], merge_only=True)
        assert e.value.code == L.ERR_ARG
        assert f"window {bad_window}:" in str(e.value), str(e.value)
        one = dict(case, clouds=case["clouds"][2 * bad_window:2 * bad_window + 2], poses=case["poses"][2 * bad_window:2 * bad_window + 2])
        with pkg.Scans(one["clouds"]) as alone:                            # the per-window path of a one-window call
            with pytest.raises(L.LvbaError) as e1:
                alone.window_ba(one["poses"], window_size=2, anchor_leaf=case["leaf"], merge_only=True)
        assert e1.value.code == L.ERR_ARG and "window 0:" in str(e1.value)
        got = scans.window_ba(case["poses"], window_size=2, anchor_leaf=0.0, merge_only=True)
        try:
            assert got["anchor_scans"].counts.tolist() == [400, 400, 400]
        finally:
            got["anchor_scans"].close()
    _assert_equals_oracle(pkg, wc.lattice_case(0.125))
    good = dict(case, clouds=[c.copy() for c in case["clouds"]])
    good["clouds"][3][57] = np.float32([0.25, 0.25, -0.5])
    _assert_equals_oracle(pkg, good)
