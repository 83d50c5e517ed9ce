"""GPU tests of the LiDAR map colouriser (lvba_colorize_*, csrc/colorize.hip; LvbaSystem::VisualizeOptComparison of the
reference): against the reference's own points3D.txt (tests/golden/ref_colorize.npz), bit for bit against the restatement
(tests/colorize_oracle.py) on seeded scenes, batching / streaming / run-to-run invariance, the pipeline entry points, the
argument checks, and the fusion_bench scale."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import colorize_oracle as co

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _mods():
    return (importlib.import_module("global-lvba_amd"), importlib.import_module("global-lvba_amd.colorize"),
            importlib.import_module("global-lvba_amd.pipeline"), importlib.import_module("global-lvba_amd.dataset"))


def run_gpu(clouds, poses, times, img_t, Rcw, tcw, intr, W, H, images, leaf, max_batch=0, calls=None):
    pkg, col, _, _ = _mods()
    with pkg.Scans(clouds) as scans, col.ColorMap(scans, poses, times, intr, W, H, leaf_size=leaf, max_batch_images=max_batch) as cm:
        m = len(img_t)
        for a, b in (calls or [(0, m)]):
            cm.add_images(img_t[a:b], Rcw[a:b], tcw[a:b], images[a:b])
        return cm.download()


# ----------------------------------------------------------------------------------------------------------- 1. the reference
def test_after_cloud_equals_reference_points3d():
    import make_golden_colorize as mg
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_colorize.npz"))
    d = mg.sequence()
    assert mg.clouds_digest(d["clouds"]) == str(g["clouds_sha256"])            # the regenerated inputs are the reference's
    W, H = int(g["width"]), int(g["height"])
    img = np.broadcast_to(co.pattern_image(W, H), (len(g["image_times"]), H, W, 3))
    xyz, rgb = run_gpu([c[:, :3] for c in d["clouds"]], g["scan_after"], g["scan_times"], g["image_times"], g["Rcw_after"],
                       g["tcw_after"], g["intr"], W, H, img, 0.01)
    rows = str(g["rows"]).split("\n")
    assert len(xyz) == int(g["n_rows"]) == len(rows)
    assert sorted(co.points3d_lines(xyz, rgb)) == rows


# ------------------------------------------------------------------------------------------------------------- 2. the oracle
def scene(seed, W=160, H=120, n_frames=8, pts=3000):
    """Scans 0.1 s apart around a camera rig, with: points duplicated across scans (two scans share pose and points), far points
    (17-300 m), points behind the cameras, points on pixel edges (u or v at k + 0.5 through an undistorted camera), random-noise
    images, and images whose window holds no scan."""
    rng = np.random.default_rng(seed)
    intr = np.array([120.0, 119.0, 79.5, 59.5, 0.0, 0.0, 0.0, 0.0]) if seed % 2 else \
        np.array([120.0, 119.0, 80.3, 60.1, -0.07616, 0.123001, -0.00113, 0.000251])
    clouds, poses = [], []
    for f in range(n_frames):
        n = pts
        p = np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.uniform(1.0, 15.0, (n, 1))], 1)
        far = rng.random(n) < 0.15
        p[far, 2] = rng.uniform(17.0, 300.0, far.sum())
        p[far, :2] *= p[far, 2:3] / 8.0
        back = rng.random(n) < 0.05
        p[back, 2] *= -1
        edge = rng.random(n) < 0.1                                            # half-integer pixels at zero distortion
        z = p[edge, 2]
        p[edge, 0] = (rng.integers(0, W, edge.sum()) + 0.5 - intr[2]) / intr[0] * z
        p[edge, 1] = (rng.integers(0, H, edge.sum()) + 0.5 - intr[3]) / intr[1] * z
        dup = rng.random(n) < 0.1                                             # repeated points inside a scan
        p[dup] = p[rng.integers(0, n, dup.sum())]
        clouds.append(p.astype(np.float32))
        ang = rng.normal(0, 0.02, 3)
        R = np.array([[1, -ang[2], ang[1]], [ang[2], 1, -ang[0]], [-ang[1], ang[0], 1]])
        R = np.linalg.qr(R)[0] * np.sign(np.diag(np.linalg.qr(R)[1]))
        poses.append(np.r_[R.reshape(-1), rng.normal(0, 0.1, 3)])
    clouds[3] = clouds[2].copy(); poses[3] = poses[2].copy()                  # duplicates across scans
    poses = np.array(poses)
    times = 10.0 + 0.1 * np.arange(n_frames)
    times[5:] += 2.0                                                          # a gap: images at 11.5 see nothing
    img_t = np.array([10.0, 10.25, 10.4, 11.5, 12.6, 12.95, 20.0, 10.7])
    m = len(img_t)
    Rcw = np.array([np.linalg.qr(np.eye(3) + rng.normal(0, 0.01, (3, 3)))[0] for _ in range(m)])
    Rcw = Rcw * np.sign(np.einsum("kii->ki", Rcw))[:, None, :]
    Rcw[0] = np.eye(3)
    tcw = rng.normal(0, 0.05, (m, 3))
    tcw[0] = 0.0
    images = rng.integers(0, 256, (m, H, W, 3), dtype=np.uint8)
    return dict(clouds=clouds, poses=poses, times=times, img_t=img_t, Rcw=Rcw, tcw=tcw, intr=intr, W=W, H=H, images=images)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("leaf", [0.0, 0.01])
def test_bitwise_equal_to_oracle(seed, leaf):
    s = scene(seed)
    args = (s["clouds"], s["poses"], s["times"], s["img_t"], s["Rcw"], s["tcw"], s["intr"], s["W"], s["H"], s["images"])
    xo, co_ = co.colorize(*args, leaf=leaf)
    xg, cg = run_gpu(*args, leaf)
    assert len(xo) > 1000
    assert xg.dtype == np.float32 and cg.dtype == np.uint8
    assert np.array_equal(xg.view(np.uint32), xo.view(np.uint32)) and np.array_equal(cg, co_)


# --------------------------------------------------------------------------------------------------------- 3. invariance
@pytest.mark.parametrize("leaf", [0.0, 0.01])
def test_same_bytes_for_any_batching(leaf):
    s = scene(5)
    args = (s["clouds"], s["poses"], s["times"], s["img_t"], s["Rcw"], s["tcw"], s["intr"], s["W"], s["H"], s["images"])
    ref = run_gpu(*args, leaf)
    assert len(ref[0]) > 1000
    m = len(s["img_t"])
    for kw in (dict(max_batch=1), dict(max_batch=3), dict(max_batch=m), dict(calls=[(0, 2), (2, 3), (3, 7), (7, m)]),
               dict(max_batch=2, calls=[(0, 5), (5, m)]), dict()):
        got = run_gpu(*args, leaf, **kw)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1]), kw


# ------------------------------------------------------------------------------------------------------ 4. pipeline entry points
def _pipeline_data():
    import test_gpu_pipeline as tp
    d = tp._dataset(n_frames=10, pts=20000, n_land=300, seed=64)
    rng = np.random.default_rng(64)
    images = rng.integers(0, 256, (len(d["img_t"]), tp.H, tp.W, 3), dtype=np.uint8)
    cfg = dict(window_size=5, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    return tp, d, images, cfg


def _check_against_oracle(out, clouds, x_before, scan_times, img_t, images, intr, W, H):
    v = out["visual"]
    for name, (x, R, t) in (("colored_after", (out["poses"], v["Rcw"], v["tcw"])),
                            ("colored_before", (x_before, v["Rcw_before"], v["tcw_before"]))):
        xo, c = co.colorize(clouds, x, scan_times, img_t, R, t, intr, W, H, images, leaf=0.01)
        xg, cg = out[name]
        assert len(xo) > 1000 and np.array_equal(xg.view(np.uint32), xo.view(np.uint32)) and np.array_equal(cg, c), name


def test_run_full_pipeline_with_images():
    _, _, pipe, _ = _mods()
    tp, d, images, cfg = _pipeline_data()
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"], d["pairs"], d["matches"])
    out = pipe.run_full_pipeline(*args, images=images, **cfg)
    _check_against_oracle(out, [c[:, :3] for c in d["clouds"]], d["odo"], d["times"], d["img_t"], images, tp.INTR, tp.W, tp.H)
    assert not np.array_equal(out["colored_after"][0], out["colored_before"][0])
    out2 = pipe.run_full_pipeline(*args, images=lambda k: images[k], **cfg)                  # the callable form
    assert np.array_equal(out2["colored_after"][1], out["colored_after"][1])
    plain = pipe.run_full_pipeline(*args, **cfg)                                              # default: no colour map
    assert "colored_after" not in plain and np.array_equal(plain["poses"], out["poses"])


def test_run_dataset_colorize(tmp_path):
    import sqlite3
    from PIL import Image
    _, _, pipe, ds = _mods()
    tp, d, images, cfg = _pipeline_data()
    root = tmp_path / "seq"
    (root / "all_pcd_body").mkdir(parents=True); (root / "all_image").mkdir()
    for t, c in zip(d["times"], d["clouds"]):
        ds.save_pcd(str(root / "all_pcd_body" / f"{t:.6f}.pcd"), np.concatenate([c[:, :3], np.zeros((len(c), 1), np.float32)], 1))
    ds.write_poses_tum(str(root / "all_pcd_body" / "lidar_poses.txt"), d["times"], d["odo"])
    for k, t in enumerate(d["img_t"]):
        mode_img = images[k][:, :, ::-1]                                   # written as RGB, read back as BGR
        if k % 3 == 1:
            Image.fromarray(np.concatenate([mode_img, np.full(mode_img.shape[:2] + (1,), 7, np.uint8)], 2), "RGBA").save(root / "all_image" / f"{t:.6f}.png")
        else:
            Image.fromarray(np.ascontiguousarray(mode_img), "RGB").save(root / "all_image" / f"{t:.6f}.png")
    ds.write_poses_tum(str(root / "all_image" / "image_poses.txt"), d["img_t"], d["odo"])
    con = sqlite3.connect(str(root / "colmap.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    for i, t in enumerate(d["img_t"]):
        kp4 = np.concatenate([d["kps"][i], np.ones((len(d["kps"][i]), 2), np.float32)], 1).astype(np.float32)
        con.execute("INSERT INTO images VALUES (?, ?)", (i + 1, f"{t:.6f}.png"))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (i + 1, kp4.shape[0], 4, kp4.tobytes()))
    for (i, j), m in zip(d["pairs"], d["matches"]):
        con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                    (ds.image_ids_to_pair_id(i + 1, j + 1), len(m), 2, np.asarray(m, np.uint32).tobytes()))
    con.commit(); con.close()
    out_dir = tmp_path / "out"
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir), colorize=True, **cfg)
    L = ds.load_dataset(str(root))
    _check_against_oracle(got, [c[:, :3] for c in L["clouds"]], L["poses"], got["scan_times"], got["image_ids"], images, tp.INTR,
                          tp.W, tp.H)
    for name in ("after", "before"):
        x, c = ds.load_pcd_xyzrgb(str(out_dir / f"colored_merged_{name}.pcd"))
        assert np.array_equal(x, got["colored_" + name][0]) and np.array_equal(c, got["colored_" + name][1])
    mine = tmp_path / "p3d.txt"
    ds.write_points3d_txt(str(mine), *got["colored_after"])
    assert (out_dir / "points3D.txt").read_text() == mine.read_text()
    rows = np.loadtxt(str(out_dir / "points3D.txt"), ndmin=2)
    assert len(rows) > 1000 and not np.all(rows[:, 4:7] == 255)


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_invalid_arguments_are_refused():
    pkg, col, _, _ = _mods()
    L = pkg._lib
    lib = ctypes.CDLL(L.LIB_PATH)                           # raw prototypes: NULL pointers go through as they are
    vp = ctypes.c_void_p
    lib.lvba_colorize_create.argtypes = [vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, ctypes.POINTER(vp)]
    lib.lvba_colorize_add_images.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp]
    lib.lvba_colorize_count.argtypes = [vp, ctypes.POINTER(ctypes.c_int64)]
    lib.lvba_colorize_download.argtypes = [vp, vp, vp]
    lib.lvba_colorize_destroy.argtypes = [vp]
    lib.lvba_colorize_destroy.restype = None
    lib.lvba_last_error.restype = ctypes.c_char_p
    s = scene(7)
    W, H = s["W"], s["H"]
    ptr = lambda a: a.ctypes.data
    poses, times, intr = np.ascontiguousarray(s["poses"]), np.ascontiguousarray(s["times"]), np.ascontiguousarray(s["intr"])
    with pkg.Scans(s["clouds"]) as scans:
        h = vp()

        def create(sc=scans._h, P=poses, T=times, I=intr, w=W, hh=H, out=True):
            h.value = None
            rc = lib.lvba_colorize_create(sc, ptr(P) if P is not None else None, ptr(T) if T is not None else None,
                                          ptr(I) if I is not None else None, w, hh, None, ctypes.byref(h) if out else None)
            return rc
        assert create(sc=None) == L.ERR_ARG and not h.value
        assert create(P=None) == L.ERR_ARG and create(T=None) == L.ERR_ARG and create(I=None) == L.ERR_ARG
        assert create(out=False) == L.ERR_ARG
        assert create(w=1) == L.ERR_ARG and create(hh=1) == L.ERR_ARG
        assert b"size" in lib.lvba_last_error()
        assert create(T=times[::-1].copy()) == L.ERR_ARG and b"ascending" in lib.lvba_last_error()
        bad = poses.copy(); bad[2, 4] = np.nan
        assert create(P=bad) == L.ERR_ARG
        badt = times.copy(); badt[1] = np.inf
        assert create(T=badt) == L.ERR_ARG
        badi = intr.copy(); badi[0] = np.nan
        assert create(I=badi) == L.ERR_ARG
        assert create() == L.OK and h.value
        m = len(s["img_t"])
        R, t = np.ascontiguousarray(s["Rcw"]), np.ascontiguousarray(s["tcw"])
        img_t, img = np.ascontiguousarray(s["img_t"]), np.ascontiguousarray(s["images"])
        assert lib.lvba_colorize_add_images(None, m, ptr(img_t), ptr(R), ptr(t), ptr(img)) == L.ERR_ARG
        assert lib.lvba_colorize_add_images(h, -1, ptr(img_t), ptr(R), ptr(t), ptr(img)) == L.ERR_ARG
        assert lib.lvba_colorize_add_images(h, m, ptr(img_t), ptr(R), ptr(t), None) == L.ERR_ARG
        assert lib.lvba_colorize_add_images(h, m, None, ptr(R), ptr(t), ptr(img)) == L.ERR_ARG
        badR = R.copy(); badR[1, 0, 0] = np.nan
        assert lib.lvba_colorize_add_images(h, m, ptr(img_t), ptr(badR), ptr(t), ptr(img)) == L.ERR_ARG
        n = ctypes.c_int64(-1)
        assert lib.lvba_colorize_count(h, ctypes.byref(n)) == L.OK and n.value == 0           # nothing was added
        assert lib.lvba_colorize_count(None, ctypes.byref(n)) == L.ERR_ARG
        assert lib.lvba_colorize_add_images(h, 0, None, None, None, None) == L.OK
        assert lib.lvba_colorize_add_images(h, m, ptr(img_t), ptr(R), ptr(t), ptr(img)) == L.OK   # still usable
        assert lib.lvba_colorize_count(h, ctypes.byref(n)) == L.OK and n.value > 1000
        assert lib.lvba_colorize_download(h, None, None) == L.ERR_ARG
        lib.lvba_colorize_destroy(h)
        lib.lvba_colorize_destroy(None)
    # a finite world point outside the packable leaf range is refused when thinning, accepted without thinning
    far = [np.array([[2.0e4, 0.0, 5.0], [0.0, 0.0, 5.0]], np.float32)]
    with pkg.Scans(far) as sc:
        with pytest.raises(L.LvbaError) as e:
            col.ColorMap(sc, np.r_[np.eye(3).reshape(-1), 0, 0, 0][None], [0.0], intr, W, H, leaf_size=0.01)
        assert e.value.code == L.ERR_ARG
        with col.ColorMap(sc, np.r_[np.eye(3).reshape(-1), 0, 0, 0][None], [0.0], intr, W, H, leaf_size=0.0) as cm:
            cm.add_images([0.0], np.eye(3)[None], np.zeros((1, 3)), np.zeros((1, H, W, 3), np.uint8))
            assert cm.count() == 1
    assert pkg._lib.load().lvba_version() == 112


# --------------------------------------------------------------------------------------------------------------- 6. scale
def test_fusion_bench_scale_three_images():
    """tools/fusion_bench.py's scene: 64 frames x 100 k points, 1280 x 1024; three sampled images, no thinning."""
    synth = importlib.import_module("global-lvba_amd.synth")
    frames, ppf, W, H = 64, 100000, 1280, 1024
    intr = np.array([646.78472, 646.65775, 313.456795 * 2, 261.399612 * 2, -0.076160, 0.123001, -0.00113, 0.000251])
    RCB = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    s = synth.make_scans(frames, ppf, room=(30, 20, 6), n_panels=0, n_blobs=0, clutter_frac=0.0, rot_sigma_deg=0.0, trans_sigma=0.0)
    poses = np.asarray(s["poses_gt"], np.float64).reshape(-1, 12)
    times = 100.0 + 0.1 * np.arange(frames)
    Rcw = np.array([RCB @ T[:9].reshape(3, 3).T for T in poses])
    tcw = np.array([-R @ T[9:] for R, T in zip(Rcw, poses)])
    pick = np.array([3, 31, 60])
    rng = np.random.default_rng(8)
    images = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    clouds = [c[:, :3] for c in s["clouds"]]
    xg, cg = run_gpu(clouds, poses, times, times[pick], Rcw[pick], tcw[pick], intr, W, H, images, 0.0)
    xo, c = co.colorize(clouds, poses, times, times[pick], Rcw[pick], tcw[pick], intr, W, H, images, leaf=0.0)
    assert len(xo) > 100000
    assert np.array_equal(xg.view(np.uint32), xo.view(np.uint32)) and np.array_equal(cg, c)
