"""GPU test of run_dataset(features="images"): the synthetic data set of tests/test_gpu_pipeline.py (its generator, imported), with
PNGs that show the room's walls under a procedural texture from the planted camera poses, and no database file.  The features
come from the images (features.py), the matches from the guided matcher, and the visual stage runs on them."""
import importlib
import sqlite3

import numpy as np
import pytest

import test_gpu_pipeline as tp

pytestmark = pytest.mark.gpu

ROOM = np.array([14.0, 10.0, 4.0])            # the room test_gpu_pipeline._dataset scans, centred at the origin
CFG = dict(window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))


def _pixel_rays():
    """the undistorted normalised ray of every pixel (the fixed-point iteration of the camera model, 8 rounds)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = tp.INTR
    v, u = np.mgrid[0:tp.H, 0:tp.W].astype(np.float64)
    xd, yd = (u - cx) / fx, (v - cy) / fy
    xu, yu = xd, yd
    for _ in range(8):
        r2 = xu * xu + yu * yu
        radial = 1.0 + k1 * r2 + k2 * r2 * r2
        xt = 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu)
        yt = p1 * (r2 + 2.0 * yu * yu) + 2.0 * p2 * xu * yu
        xu, yu = (xd - xt) / radial, (yd - yt) / radial
    return np.stack([xu, yu, np.ones_like(xu)], -1)


def _texture(P, rng_seed=5):
    """a smooth random pattern on the walls: 28 plane waves of 0.12 .. 0.7 m wavelength, evaluated at the 3-D point"""
    rng = np.random.default_rng(rng_seed)
    out = np.zeros(P.shape[:-1])
    for _ in range(28):
        k = rng.normal(size=3)
        k *= (2 * np.pi / rng.uniform(0.12, 0.7)) / np.linalg.norm(k)
        out += rng.uniform(0.5, 1.0) * np.sin(P @ k + rng.uniform(0, 2 * np.pi))
    return out


def render_views(d):
    """uint8 [H, W] per camera: the first wall every pixel's ray meets, under the texture"""
    rays = _pixel_rays()
    views = []
    for R, t in zip(d["Rcw_gt"], d["tcw_gt"]):
        C = -R.T @ t
        D = rays @ R                                                   # R^T ray, per pixel
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.min(np.where(D != 0.0, (np.sign(D) * ROOM / 2 - C) / D, np.inf), axis=-1)
        g = 128.0 + 22.0 * _texture(C + s[..., None] * D)
        views.append(np.clip(np.rint(g), 0, 255).astype(np.uint8))
    return views


def write_dataset(root, d, views=None, db=False):
    from PIL import Image
    ds = importlib.import_module("global-lvba_amd.dataset")
    (root / "all_pcd_body").mkdir(parents=True); (root / "all_image").mkdir()
    for t, c in zip(d["times"], d["clouds"]):
        ds.save_pcd(str(root / "all_pcd_body" / f"{t:.6f}.pcd"), np.concatenate([c[:, :3], np.zeros((len(c), 1), np.float32)], 1))
    ds.write_poses_tum(str(root / "all_pcd_body" / "lidar_poses.txt"), d["times"], d["odo"])
    for k, t in enumerate(d["img_t"]):
        if views is None:
            (root / "all_image" / f"{t:.6f}.png").write_bytes(b"")
        else:
            Image.fromarray(views[k]).save(str(root / "all_image" / f"{t:.6f}.png"))
    ds.write_poses_tum(str(root / "all_image" / "image_poses.txt"), d["img_t"], d["odo"])
    if db:
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


def test_pipeline_from_images_without_a_database(pkg, tmp_path):
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = tp._dataset(n_frames=20, pts=30000, n_land=30, seed=63)
    root = tmp_path / "seq"
    write_dataset(root, d, views=render_views(d))
    args = (str(root), "no_such.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI)
    with pytest.raises(ValueError, match="matching"):
        pipe.run_dataset(*args, features="images", matching="db", **CFG)
    out = pipe.run_dataset(*args, features="images", matching="guided", feature_opts=dict(max_features=2000), **CFG)
    assert not (root / "no_such.db").exists()
    n_matches = sum(len(m) for m in out["matches"])
    v = out["visual"]
    tr = v["trace"]
    print(f"features from images: {len(out['pairs'])} matched pairs, {n_matches} matches, {v['n_components']} components, "
          f"{len(v['landmarks'])} landmarks, cost {tr[0]['cost']:.4e} -> {tr[-1]['cost']:.4e}" if tr else "no tracks")
    assert len(out["pairs"]) >= 19 and n_matches > 500                   # at least the neighbours in time see the same wall
    assert v["n_components"] > 50 and len(v["landmarks"]) > 20 and (v["track_status"] > 0).sum() > 20
    assert len(tr) >= 1 and all(np.isfinite(s["cost"]) for s in tr) and np.isfinite(v["tcw"]).all()
    # the matches are geometry, not chance: the fused landmarks lie on the walls
    X = v["landmarks_before"]
    wall = np.min(np.abs(np.abs(X) - ROOM / 2), axis=1)
    assert np.median(wall) < 0.1


def test_features_db_is_the_path_of_before(pkg, tmp_path):
    """features="db" spelled out gives, byte for byte, what the call without the argument gives on the directory fixture of
    test_gpu_pipeline.py (key points and matches from the database)."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = tp._dataset(n_frames=12, pts=40000, n_land=400, seed=62)
    root = tmp_path / "seq"
    write_dataset(root, d, db=True)
    args = (str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI)
    a = pipe.run_dataset(*args, **CFG)
    b = pipe.run_dataset(*args, features="db", **CFG)
    assert a["poses"].tobytes() == b["poses"].tobytes()
    va, vb = a["visual"], b["visual"]
    assert va["n_components"] == vb["n_components"] > 100
    for key in ("track_status", "Rcw", "tcw", "landmarks", "landmark_valid", "obs_uv"):
        assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), key
    assert [s["cost"] for s in va["trace"]] == [s["cost"] for s in vb["trace"]]
