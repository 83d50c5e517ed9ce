"""GPU parity test of the window-BA stage (lvba_window_ba) against oracle/window_oracle.py: same scans, same odometry.

NOTE on what "the oracle" is here: the reference's down_sampling_voxel2 emits its survivors in std::unordered_map order
(unspecified); both the product and window_oracle.py emit them SORTED BY VOXEL KEY instead.  The oracle in that KEY ORDER is
what tests/test_ref_system.py holds against the reference's own runLidarBA (poses to 4e-13), so the tests below compare with
a re-ordered restatement, and anchor clouds as point SETS -- hence the names.

Per window: voxel counts and skip decisions exact; optimised poses / relative poses to 1e-7 (they inherit the LM parity
of tests/test_gpu_balm.py); anchor clouds: the fp32 points that survive down_sampling_voxel2.  A relative pose that differs
by 1e-9 can move a transformed coordinate across an fp32 rounding boundary, so clouds are compared as point sets with a
1e-5 m tolerance and a 0.2 % budget for flipped survivors.
That budget is for the poses alone.  The merge itself is deterministic given the relative poses a call returns, so beside the
comparison with the oracle every test holds the anchor clouds, point for point and in order, to the replay of the merge from
the call's own rel_poses (_assert_replay; tests/test_gpu_window_merge.py holds the merge to the oracle itself on exact inputs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _compare_clouds(a, b):
    assert abs(len(a) - len(b)) <= max(2, 0.002 * len(b))
    # both are sorted by voxel key; match greedily through a KD-free trick: sort rows lexicographically after rounding
    from scipy.spatial import cKDTree
    d, _ = cKDTree(b).query(a, k=1)
    assert np.mean(d > 1e-5) <= 0.002, float(np.mean(d > 1e-5))


def _assert_replay(clouds, got, window_size, leaf, pts=None):
    """The merge stage is deterministic given the relative poses the call returned (pose_apply_f32 and leaf_key_of are compiled
    without contraction, tests/window_merge_cases.py restates them): the anchor clouds equal the replay point for point, in
    order, whatever the LM did to the poses and whichever windows were skipped.  pts: the clouds, if already downloaded."""
    import window_merge_cases as wc
    replay = wc.replay_anchor_clouds(clouds, got["rel_poses"], got["windows"], window_size, leaf)
    if pts is None:
        pts = [got["anchor_scans"].download(a) for a in range(got["anchor_scans"].n_frames)]
    assert len(pts) == len(replay) == sum(not w["skipped"] for w in got["windows"])
    for a, (p, r) in enumerate(zip(pts, replay)):
        np.testing.assert_array_equal(p, r, err_msg=f"anchor {a}")


@pytest.mark.parametrize("use_rel", [True, False])
@pytest.mark.parametrize("leaf", [0.05, 0.0])
def test_window_ba_matches_key_ordered_oracle_clouds_as_point_sets(pkg, synth, use_rel, leaf):
    from oracle import window_oracle as wo
    s = synth.make_scans(10, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=31, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    ratio = np.float32([0.3, 0.1, 0.06, 0.03])
    ref = wo.run_window_ba(s["clouds"], s["poses"], 4, 1.0, ratio, leaf, use_rel)
    with pkg.Scans(s["clouds"]) as scans:
        got = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, eigen_ratio_array=ratio, anchor_leaf=leaf,
                              use_rel=use_rel)
    assert len(got["windows"]) == len(ref["windows"]) == 3
    for g, r in zip(got["windows"], ref["windows"]):
        assert (g["start"], g["n_frames"], g["n_voxels"], bool(g["skipped"])) == (r["start"], r["n"], r["n_voxels"], r["skipped"])
        assert g["n_iter"] == len(r["trace"])
        assert abs(g["cost_first"] - r["trace"][0][1]) <= 1e-9 * r["trace"][0][1]
    np.testing.assert_array_equal(got["anchor_index"], ref["anchor_index"])
    assert np.abs(got["window_poses"] - ref["window_poses"]).max() < 1e-7
    assert np.abs(got["rel_poses"] - ref["rel_poses"]).max() < 1e-7
    np.testing.assert_array_equal(got["anchor_poses"], ref["anchor_poses"])
    asc = got["anchor_scans"]
    assert asc.n_frames == len(ref["anchor_clouds"])
    for a in range(asc.n_frames):
        _compare_clouds(asc.download(a), ref["anchor_clouds"][a])
    _assert_replay(s["clouds"], got, 4, leaf)
    # the LM did something: the optimised windows moved away from the odometry
    assert np.abs(got["window_poses"] - s["poses"]).max() > 1e-4
    # the anchors feed the global stage directly: a map over the anchor clouds builds and refines
    with asc.voxel_map(got["anchor_poses"], 1.0) as m:
        assert m.info["n_voxels"] > 50
    asc.close()


def test_window_skip_rule_and_identity_rel(pkg, synth):
    """A window with fewer than 3 plane voxels per frame is skipped: no anchor, index -1, identity relative pose."""
    s = synth.make_scans(4, 4000, room=(8, 6, 3), n_panels=4, seed=5)
    rng = np.random.default_rng(0)
    clouds = list(s["clouds"])
    clouds[2] = rng.uniform(-1, 1, (300, 3)).astype(np.float32)        # window 1 = frames 2,3: volume noise only
    clouds[3] = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    with pkg.Scans(clouds) as scans:
        got = scans.window_ba(s["poses"], window_size=2, voxel_size=1.0, anchor_leaf=0.05)
    w = got["windows"]
    assert not w[0]["skipped"] and w[1]["skipped"] and w[1]["anchor"] == -1
    assert got["anchor_index"].tolist() == [0, 0, -1, -1]
    I12 = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    np.testing.assert_array_equal(got["rel_poses"][2:], np.tile(I12, (2, 1)))
    np.testing.assert_array_equal(got["window_poses"][2:], s["poses"][2:])
    assert got["anchor_scans"].n_frames == 1
    _assert_replay(clouds, got, 2, 0.05)
    got["anchor_scans"].close()


def test_skipped_window_after_four_merged_takes_the_code_of_a_third_bit(pkg, synth):
    """20 frames, windows of 4: four windows merge and the last one is skipped.  In the joint pass the skipped window's points
    get the code G = 4, a power of two, above the codes 0 .. 3 of the merged ones: the window code needs three bits, not the two
    that G - 1 has (merge_run: cbits).  With a bit too few the code 4 would alias window 0's, and the skipped window's points
    would sort into its leaves.  Held to the oracle as the neighbouring tests are, and to the replay point for point."""
    from oracle import window_oracle as wo
    s = synth.make_scans(20, 6000, room=(10, 8, 4), origin=(2.0, -1.0, 0.4), n_panels=8, seed=45, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    clouds = [c.copy() for c in s["clouds"]]
    for f in range(16, 20):
        clouds[f] = clouds[f][:40]                                          # window 4 (frames 16..19) has too few planes: skipped
    ratio = np.float32([0.3, 0.1, 0.06, 0.03])
    ref = wo.run_window_ba(clouds, s["poses"], 4, 1.0, ratio, 0.05)
    with pkg.Scans(clouds) as scans:
        got = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, eigen_ratio_array=ratio, anchor_leaf=0.05)
    asc = got["anchor_scans"]
    try:
        assert [w["skipped"] for w in got["windows"]] == [int(w["skipped"]) for w in ref["windows"]] == [0, 0, 0, 0, 1]
        assert [w["anchor"] for w in got["windows"]] == [0, 1, 2, 3, -1]
        np.testing.assert_array_equal(got["anchor_index"], ref["anchor_index"])
        np.testing.assert_array_equal(got["anchor_poses"], ref["anchor_poses"])
        assert np.abs(got["rel_poses"] - ref["rel_poses"]).max() < 1e-7
        assert asc.n_frames == len(ref["anchor_clouds"]) == 4
        for a in range(4):
            _compare_clouds(asc.download(a), ref["anchor_clouds"][a])
        _assert_replay(clouds, got, 4, 0.05)
    finally:
        asc.close()


@pytest.mark.parametrize("window_enable", [True, False])
def test_lidar_ba_pipeline_matches_key_ordered_oracle(pkg, synth, window_enable):
    """lvba_lidar_ba = runLidarBA's compute: window BA -> anchors -> stage 1 -> stage 2 -> composed frame poses."""
    from oracle import window_oracle as wo
    s = synth.make_scans(12, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=41, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    kw = dict(window_enable=window_enable, window_size=4, anchor_leaf=0.05, stage_voxel_size=(1.0, 0.5))
    ref, rrep = wo.run_lidar_ba(s["clouds"], s["poses"], **kw)
    with pkg.Scans(s["clouds"]) as scans:
        got, rep = scans.lidar_ba(s["poses"], **kw)
    assert rep["n_anchors"] == rrep["n_anchors"] == (3 if window_enable else 12)
    for st in rrep["stages"]:
        i = st["stage"]
        assert rep["stage_ran"][i] == 1
        if window_enable:
            # anchor clouds may differ by a few fp32 survivors (see above): voxel counts agree to a fraction of a percent
            assert abs(rep["stage_voxels"][i] - st["n_voxels"]) <= max(3, 0.01 * st["n_voxels"])
        else:
            assert rep["stage_voxels"][i] == st["n_voxels"]
            assert rep["stage_iters"][i] == len(st["trace"])
            assert abs(rep["stage_cost_first"][i] - st["trace"][0][1]) <= 1e-9 * st["trace"][0][1]
    tol = 1e-7 if not window_enable else 2e-4      # with windows, the stages see slightly different anchor clouds
    assert np.abs(got - ref).max() < tol
    # and the pipeline improved the trajectory: closer to ground truth than the odometry it started from
    def err(x):
        return np.abs(x[:, 9:] - s["poses_gt"][:, 9:]).mean()
    assert err(got) < err(s["poses"])


def test_window_threads_give_identical_results(pkg, synth, monkeypatch):
    """Windows are worked through by several host threads (LVBA_WINDOW_THREADS, default 4); every window's arithmetic is
    independent of the others, so the outputs must be bitwise those of the single-threaded run -- poses, relative poses,
    anchor numbering (with a skipped window in between) and the anchor clouds."""
    s = synth.make_scans(22, 6000, room=(10, 8, 4), origin=(2.0, -1.0, 0.4), n_panels=8, seed=41, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    clouds = [c.copy() for c in s["clouds"]]
    for f in range(8, 12):
        clouds[f] = clouds[f][:40]                                          # window 2 (frames 8..11) has too few planes: skipped
    outs = {}
    for thr in ("1", "4"):
        monkeypatch.setenv("LVBA_WINDOW_THREADS", thr)
        with pkg.Scans(clouds) as scans:
            got = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, anchor_leaf=0.05)
        pts = [got["anchor_scans"].download(a) for a in range(len(got["anchor_poses"]))]
        got["anchor_scans"].close()
        outs[thr] = (got, pts)
    a, b = outs["1"], outs["4"]
    assert [w["skipped"] for w in a[0]["windows"]] == [0, 0, 1, 0, 0, 0]
    for k in ("window_poses", "rel_poses", "anchor_index", "anchor_poses"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    assert [w["anchor"] for w in a[0]["windows"]] == [w["anchor"] for w in b[0]["windows"]] == [0, 1, -1, 2, 3, 4]
    assert len(a[1]) == len(b[1]) == 5
    for p, q in zip(a[1], b[1]):
        np.testing.assert_array_equal(p, q)
    _assert_replay(clouds, a[0], 4, 0.05, a[1])


def test_windows_in_lock_step_equal_one_at_a_time(pkg, synth):
    """lm_mode 0 (default): the damping_iter of all windows advances in lock-step on ONE grouped problem (one evaluation, one band
    factorisation with a damping value per window, one cost pass per LM iteration for all windows -- lvba_balm_refine_groups);
    lm_mode 1: one window at a time, as the reference does (src/lvba_system.cpp:232-302).  The windows are independent either
    way: same skipped windows, same iteration counts, poses to 1e-9, and anchor clouds that are the same point sets up to the
    fp32 write-back of points moved by 1e-9."""
    s = synth.make_scans(22, 6000, room=(10, 8, 4), origin=(2.0, -1.0, 0.4), n_panels=8, seed=43, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    clouds = [c.copy() for c in s["clouds"]]
    for f in range(8, 12):
        clouds[f] = clouds[f][:40]                                          # window 2 (frames 8..11) is skipped
    outs = []
    for mode in (0, 1):
        with pkg.Scans(clouds) as scans:
            got = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, anchor_leaf=0.05, lm_mode=mode)
        pts = [got["anchor_scans"].download(a) for a in range(len(got["anchor_poses"]))]
        got["anchor_scans"].close()
        outs.append((got, pts))
    (a, pa), (b, pb) = outs
    assert [w["skipped"] for w in a["windows"]] == [w["skipped"] for w in b["windows"]] == [0, 0, 1, 0, 0, 0]
    assert [w["n_iter"] for w in a["windows"]] == [w["n_iter"] for w in b["windows"]]
    assert max(w["n_iter"] for w in a["windows"]) >= 2
    for wa, wb in zip(a["windows"], b["windows"]):
        if not wa["skipped"]:
            assert abs(wa["cost_first"] - wb["cost_first"]) <= 1e-9 * wb["cost_first"]
            assert abs(wa["cost_last"] - wb["cost_last"]) <= 1e-8 * wb["cost_last"]
    assert np.abs(a["window_poses"] - b["window_poses"]).max() <= 1e-9
    assert np.abs(a["rel_poses"] - b["rel_poses"]).max() <= 1e-9
    np.testing.assert_array_equal(a["anchor_index"], b["anchor_index"])
    np.testing.assert_array_equal(a["anchor_poses"], b["anchor_poses"])
    for p, q in zip(pa, pb):
        assert abs(len(p) - len(q)) <= 0.002 * len(q)
    _assert_replay(clouds, a, 4, 0.05, pa)
    _assert_replay(clouds, b, 4, 0.05, pb)


def test_merge_only_matches_the_anchor_merge_of_the_visual_stage(pkg, synth):
    """lvba_window_opts.merge_only = the anchor clouds optimizeCameraPoses rebuilds from the refined poses
    (src/lvba_system.cpp:1466-1489: no window BA, every scan moved into the frame of its window's first scan with the poses
    given, down_sampling_voxel2) against oracle/window_oracle.merge_anchors -- itself held against the reference's own function
    through the planes it yields (tests/test_ref_system.py)."""
    from oracle import window_oracle as wo
    s = synth.make_scans(10, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=33, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    ap, ac = wo.merge_anchors(s["clouds"], s["poses"], 4, 0.05)
    with pkg.Scans(s["clouds"]) as scans:
        got = scans.window_ba(s["poses"], window_size=4, anchor_leaf=0.05, merge_only=True)
    asc = got["anchor_scans"]
    try:
        np.testing.assert_array_equal(got["anchor_poses"], ap)
        assert got["anchor_index"].tolist() == [0] * 4 + [1] * 4 + [2] * 2
        assert asc.n_frames == len(ac) == 3
        for a in range(3):
            _compare_clouds(asc.download(a), ac[a])
        _assert_replay(s["clouds"], got, 4, 0.05)
    finally:
        asc.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_window_stage_over_several_shares_equals_one_device(pkg, synth, devices):
    """lvba_window_ba_multi: the windows of a sequence dealt out to several GPUs in contiguous runs of whole windows
    (lvba_window_split = the thread split of bavoxel.hpp:621-624 on windows), one host thread per share, anchors gathered on the
    first device.  On the one GPU of the test box the shares all sit on device 0 (as the multi-rank tests do): everything above
    the device id -- the split, the concurrent host threads with their own handles and streams, the re-numbering of anchors with a
    skipped window in a middle share, the gathered anchor scan set -- is the code a multi-GPU node runs.  With lm_mode 1 every
    window is its own problem, so the result must be BITWISE the single-share one; with the lock-step grouped LM (default) the
    groups a window shares a factorisation with change, and the results agree to rounding."""
    s = synth.make_scans(26, 6000, room=(10, 8, 4), origin=(2.0, -1.0, 0.4), n_panels=8, seed=47, rot_sigma_deg=0.1,
                         trans_sigma=0.03)
    clouds = [c.copy() for c in s["clouds"]]
    for f in range(12, 16):
        clouds[f] = clouds[f][:40]                                          # window 3 (frames 12..15) is skipped
    for mode in (1, 0):
        with pkg.Scans(clouds) as scans:
            one = scans.window_ba(s["poses"], window_size=4, voxel_size=1.0, anchor_leaf=0.05, lm_mode=mode)
        p1 = [one["anchor_scans"].download(a) for a in range(len(one["anchor_poses"]))]
        one["anchor_scans"].close()
        got = pkg.Scans.window_ba_multi(clouds, s["poses"], devices, window_size=4, voxel_size=1.0, anchor_leaf=0.05, lm_mode=mode)
        pm = [got["anchor_scans"].download(a) for a in range(len(got["anchor_poses"]))]
        got["anchor_scans"].close()
        nw = 7                                                              # 26 frames: six windows of 4 and one of 2
        fb = got["frame_begin"]
        assert fb[0] == 0 and fb[-1] == 26 and all(b % 4 == 0 for b in fb[:-1]) and len(set(fb)) == len(devices) + 1
        assert [w["skipped"] for w in got["windows"]] == [w["skipped"] for w in one["windows"]] == [0, 0, 0, 1, 0, 0, 0]
        assert [w["start"] for w in got["windows"]] == [4 * k for k in range(nw)]
        assert [w["anchor"] for w in got["windows"]] == [w["anchor"] for w in one["windows"]] == [0, 1, 2, -1, 3, 4, 5]
        np.testing.assert_array_equal(got["anchor_index"], one["anchor_index"])
        np.testing.assert_array_equal(got["anchor_poses"], one["anchor_poses"])
        assert len(pm) == len(p1) == 6
        if mode == 1:
            for k in ("window_poses", "rel_poses"):
                np.testing.assert_array_equal(got[k], one[k])
            for p, q in zip(pm, p1):
                np.testing.assert_array_equal(p, q)
        else:
            assert np.abs(got["window_poses"] - one["window_poses"]).max() <= 1e-9
            assert np.abs(got["rel_poses"] - one["rel_poses"]).max() <= 1e-9
            for p, q in zip(pm, p1):
                assert abs(len(p) - len(q)) <= 0.002 * len(q)
        _assert_replay(clouds, one, 4, 0.05, p1)
        _assert_replay(clouds, got, 4, 0.05, pm)


def test_lidar_stage_with_the_windows_over_several_shares(pkg, synth):
    """lvba_lidar_ba_multi: runLidarBA with its window stage dealt out to several shares (on the test box all on device 0), the
    two global stages on the first share's device over the gathered anchors.  With one window per problem (the default batching
    is per share, so the grouped LM sees other groups than in the one-share run) the anchors differ at rounding level only: same
    anchors, same stage sizes to a fraction of a percent, final poses to the tolerance the one-device test holds against the oracle."""
    s = synth.make_scans(16, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=43, rot_sigma_deg=0.1, trans_sigma=0.03)
    kw = dict(window_size=4, anchor_leaf=0.05, stage_voxel_size=(1.0, 0.5))
    with pkg.Scans(s["clouds"]) as scans:
        one, rep1 = scans.lidar_ba(s["poses"], **kw)
    got, rep = pkg.Scans.lidar_ba_multi(s["clouds"], s["poses"], (0, 0), **kw)
    assert rep["n_frames"] == 16 and rep["n_windows"] == rep1["n_windows"] == 4 and rep["n_anchors"] == rep1["n_anchors"] == 4
    for i in range(2):
        assert rep["stage_ran"][i] == rep1["stage_ran"][i] == 1
        assert abs(rep["stage_voxels"][i] - rep1["stage_voxels"][i]) <= max(3, 0.01 * rep1["stage_voxels"][i])
    assert np.abs(got - one).max() < 2e-4
