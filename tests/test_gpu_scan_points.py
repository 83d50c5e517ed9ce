"""GPU test of the scan-set front ends on ONE scan set with empty frames: the frame of a point, the pose and the keys are
csrc/scan_points.h for all of them, and every front end is held here against the oracle its own GPU test uses, with that
test's equality (bit for bit wherever that test asserts bit equality).

The set: frame counts [0, 1, 0, 0, 65, 3, 0] -- empty frames at both ends and in a row, a frame of one point, a frame longer
than a wavefront --, points random within +-20 m, random rigid poses.  Frame 5 holds two constructed points: its pose is a signed
axis permutation with a dyadic translation, so R p + t is exact.  One point lies exactly on a voxel face in the world (x = 3.0);
the other has a negative world coordinate whose quotient is an exact negative integer (-2.0): where "minus one for negatives"
bites.  In their own frame they are (8.125, -1.5, 11.25) and (1.0, 3.5, 9.5): -1.5 is exactly -3 leaves of 0.5 m, 1.0 and 3.5
lie on leaf faces.  Frame 5 leads the second window of the merge (window_size 5), so they reach the leaf key as they are.

Empty frames: none of the calls below has an argument check that refuses them (lvba_scans_create asks for counts >= 0, the
map-quality call for n_frames >= 1; the same checks before the rules moved into scan_points.h), so every call is compared with
its oracle and none is expected to refuse."""
import importlib

import numpy as np
import pytest

import colorize_oracle as co
import mapq_oracle as mo

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 0, 0, 65, 3, 0]
TIMES = 10.0 + 0.4 * np.arange(7)
IMG_T = np.array([10.2, 12.0])            # +-0.5 s: frames [0, 2) and [4, 7)
INTR = np.array([20.0, 21.0, 32.0, 24.0, 0.01, -0.002, 0.001, -0.0005])
W, H = 64, 48


def scene():
    rng = np.random.default_rng(7)
    poses = []
    for f in range(7):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        poses.append(np.r_[q.reshape(-1), rng.uniform(-3, 3, 3)])
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])   # det +1
    t = np.array([1.5, -4.0, 2.0])
    poses[5] = np.r_[P.reshape(-1), t]
    clouds = [rng.uniform(-20, 20, (n, 3)).astype(np.float32) for n in COUNTS]
    on_face, negative = np.array([3.0, 7.25, -6.125]), np.array([-2.0, 5.5, 1.0])
    clouds[5][0] = P.T @ (on_face - t)       # (8.125, -1.5, 11.25): exact
    clouds[5][1] = P.T @ (negative - t)      # (1.0, 3.5, 9.5): exact
    assert clouds[5][0].tolist() == [8.125, -1.5, 11.25] and clouds[5][1].tolist() == [1.0, 3.5, 9.5]
    assert np.array_equal(clouds[5][:2].astype(np.float64) @ P.T + t, [on_face, negative])
    cams = []
    for m in range(2):                        # cameras at the origin looking along +z and +x
        R = np.eye(3) if m == 0 else np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
        cams.append(R)
    images = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return dict(clouds=clouds, poses=np.array(poses), Rcw=np.array(cams), tcw=np.zeros((2, 3)), images=images)


@pytest.fixture(scope="module")
def case(pkg):
    s = scene()
    with pkg.Scans(s["clouds"]) as scans:
        yield dict(s, scans=scans)


@pytest.mark.parametrize("begin,n", [(0, 7), (3, 3)])
def test_voxel_map(case, begin, n):
    from oracle import voxel_oracle as vo
    poses = case["poses"][begin:begin + n]
    surf_map, vox = vo.build(case["clouds"][begin:begin + n], poses, 1.0)
    off_ref, idx_ref, cl_ref = vo.pack(vox)
    with case["scans"].voxel_map(poses, 1.0, frame_begin=begin, n_frames=n) as m:
        assert m.info["n_points"] == sum(COUNTS[begin:begin + n])
        assert m.info["n_roots"] == len(surf_map) and m.info["n_voxels"] == len(vox)
        if len(vox):
            off, idx, cl, key = m.export()
            np.testing.assert_array_equal(off, off_ref)
            np.testing.assert_array_equal(idx, idx_ref)
            np.testing.assert_array_equal(cl, cl_ref)


def test_window_merge_and_downsample(case):
    from oracle import window_oracle as wo
    from test_gpu_window import _compare_clouds
    ap, ac = wo.merge_anchors(case["clouds"], case["poses"], 5, 0.5)
    got = case["scans"].window_ba(case["poses"], window_size=5, anchor_leaf=0.5, merge_only=True)
    asc = got["anchor_scans"]
    try:
        np.testing.assert_array_equal(got["anchor_poses"], ap)
        assert got["anchor_index"].tolist() == [0] * 5 + [1] * 2
        assert asc.n_frames == len(ac) == 2
        for a in range(2):
            _compare_clouds(asc.download(a), ac[a])
        # the window led by frame 5: its two constructed points survive as they are, each alone in its leaf
        assert all((asc.download(1) == p).all(1).any() for p in case["clouds"][5][:2])
    finally:
        asc.close()


def test_depth_render(case):
    from oracle import fusion_oracle as fo
    vis = importlib.import_module("global-lvba_amd.visual")
    want = fo.render_depth(case["clouds"], case["poses"], TIMES, IMG_T, case["Rcw"], case["tcw"], INTR, W, H)
    assert (want[1] > 0).sum() > 5                                          # frames [0, 2) hold one point, [4, 7) 68
    with vis.DepthImages.render(case["scans"], case["poses"], TIMES, IMG_T, case["Rcw"], case["tcw"], INTR, W, H) as d:
        for m in range(2):
            got = d.download(m)
            assert got.shape == want[m].shape and np.array_equal(got.view(np.uint32), want[m].view(np.uint32))


@pytest.mark.parametrize("leaf", [0.0, 0.5])
def test_colorize(case, leaf):
    col = importlib.import_module("global-lvba_amd.colorize")
    args = (TIMES, IMG_T, case["Rcw"], case["tcw"], INTR, W, H, case["images"])
    xo, co_ = co.colorize(case["clouds"], case["poses"], *args, leaf=leaf)
    assert len(xo) > 5
    with col.ColorMap(case["scans"], case["poses"], TIMES, INTR, W, H, leaf_size=leaf) as cm:
        cm.add_images(IMG_T, case["Rcw"], case["tcw"], case["images"])
        xg, cg = cm.download()
    assert np.array_equal(xg.view(np.uint32), xo.view(np.uint32)) and np.array_equal(cg, co_)


@pytest.mark.parametrize("begin,n", [(0, 7), (4, 2)])
def test_map_quality(case, begin, n):
    mq = importlib.import_module("global-lvba_amd.mapq")
    radius, min_n = 12.0, 4                                                  # a few to a few dozen neighbours per query
    poses = case["poses"][begin:begin + n]
    world = mo.world_points(case["clouds"][begin:begin + n], poses)
    ref = mo.metrics(world, radius, min_n)
    got = mq.map_quality_scans(case["scans"], poses, radius=radius, min_neighbors=min_n, frame_begin=begin, n_frames=n, per_point=True)
    mo.check_parity(got, ref, radius)
    assert (got["n_points"], got["n_queries"], got["n_valid"]) == (len(world), len(world), ref["n_valid"]) and ref["n_valid"] > 0
    for k in ("mme", "mpv", "mean_neighbors"):
        assert abs(got[k] - ref[k]) <= 1e-10 * abs(ref[k]), (k, got[k], ref[k])
