"""GPU test of the pipeline hook of the dynamic-point removal (pipeline.run_full_pipeline(remove_dynamic=...),
pipeline.remove_dynamic): the smallest synthetic sequence of the pipeline tests (tests/test_gpu_colorize.py's, 10 frames of
20 000 points) with a planted mover -- a cube of 0.6 m that crosses the middle of the room by 0.35 m per frame, 400 points on its
surface in every frame."""
import importlib

import numpy as np
import pytest

import dynamic_oracle as do

pytestmark = pytest.mark.gpu

HALF, STEP, PER_FRAME = 0.3, 0.35, 400


def _center(k):
    return np.array([-1.6 + STEP * k, 0.2, 0.1])


def _dataset():
    import test_gpu_pipeline as tp
    d = tp._dataset(n_frames=10, pts=20000, n_land=300, seed=64)
    rng = np.random.default_rng(640)
    clouds, mover = [], []
    for k, (c, T) in enumerate(zip(d["clouds"], d["gt"])):
        u = rng.uniform(-HALF, HALF, (PER_FRAME, 3))
        face, side = rng.integers(0, 3, PER_FRAME), rng.integers(0, 2, PER_FRAME)
        u[np.arange(PER_FRAME), face] = np.where(side == 1, HALF, -HALF)                   # on the surface of the cube
        body = ((_center(k) + u - T[9:]) @ T[:9].reshape(3, 3)).astype(np.float32)        # R^T (w - t)
        clouds.append(np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32)[:, :3], body])))
        mover.append(np.r_[np.zeros(len(c), bool), np.ones(PER_FRAME, bool)])
    rng = np.random.default_rng(64)
    images = rng.integers(0, 256, (len(d["img_t"]), tp.H, tp.W, 3), dtype=np.uint8)
    cfg = dict(window_size=5, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4))
    args = (clouds, d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"], d["pairs"], d["matches"])
    return args, cfg, images, clouds, np.concatenate(mover)


def _rows(xyz):
    return np.ascontiguousarray(xyz, np.float32).view(np.dtype((np.void, 12))).reshape(-1)


def _same(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


MQ = ("n_points", "n_queries", "n_valid", "mme", "mpv", "mean_neighbors")


def test_pipeline_removes_the_mover_from_the_map_products(pkg):
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    dyn = importlib.import_module("global-lvba_amd.dynamic")
    mq = importlib.import_module("global-lvba_amd.mapq")
    args, cfg, images, clouds, mover = _dataset()
    on = pipe.run_full_pipeline(*args, remove_dynamic=True, map_quality=True, images=images, **cfg)
    none = pipe.run_full_pipeline(*args, remove_dynamic=None, map_quality=True, images=images, **cfg)
    plain = pipe.run_full_pipeline(*args, map_quality=True, images=images, **cfg)
    # off: every output as without the argument
    assert "dynamic" not in none and "dynamic" not in plain and sorted(none) == sorted(plain)
    _same(none, plain, ("poses", "poses_before"))
    _same(none["visual"], plain["visual"], ("Rcw", "tcw", "landmarks", "landmark_valid", "track_status"))
    for name in ("colored_after", "colored_before"):
        assert none[name][0].tobytes() == plain[name][0].tobytes() and none[name][1].tobytes() == plain[name][1].tobytes()
    for name in ("after", "before"):
        assert {k: none["map_quality"][name][k] for k in MQ[:3]} == {k: plain["map_quality"][name][k] for k in MQ[:3]}
        _same(none["map_quality"][name], plain["map_quality"][name], MQ[3:])
    # on: the stages before the map products are untouched, and the report is what a direct call gives
    _same(on, plain, ("poses", "poses_before"))
    _same(on["visual"], plain["visual"], ("Rcw", "tcw", "landmarks", "landmark_valid", "track_status"))
    rep = on["dynamic"]
    ref = do.labels(clouds, on["poses"])
    differ = int((rep["label"] != ref["label"]).sum())
    print(f"points {rep['n_points']}, judged {rep['n_judged']}, dynamic {rep['n_dynamic']} (oracle {ref['n_dynamic']}, labels that differ "
          f"{differ}, oracle margin {ref['margin']:.1e}); of the {int(mover.sum())} mover points the oracle labels "
          f"{int(ref['label'][mover].sum())}, of the room's {int(ref['label'][~mover].sum())}; ms {rep['ms']}")
    assert rep["n_points"] == len(mover) == 10 * 20400 and rep["n_dynamic"] == int(rep["label"].sum()) > 0
    assert list(rep["per_frame"]) == [int(x.sum()) for x in np.split(rep["label"], 10)]
    with pkg.Scans(clouds) as sc:
        static, direct = pipe.remove_dynamic(sc, on["poses"])
        with static:
            for k in ("label", "n_free", "n_support"):
                assert direct[k].tobytes() == rep[k].tobytes()
            assert int(static.counts.sum()) == rep["n_points"] - rep["n_dynamic"]
            q = {"after": mq.map_quality_scans(static, on["poses"]), "before": mq.map_quality_scans(static, args[1])}
        with dyn.static_scans(sc, rep["label"]) as again:
            q2 = mq.map_quality_scans(again, on["poses"])
    for name in ("after", "before"):
        assert {k: on["map_quality"][name][k] for k in MQ[:3]} == {k: q[name][k] for k in MQ[:3]}
        _same(on["map_quality"][name], q[name], MQ[3:])
    _same(q2, q["after"], MQ[3:])
    assert on["map_quality"]["after"]["n_points"] == rep["n_points"] - rep["n_dynamic"] < plain["map_quality"]["after"]["n_points"]
    # the coloured map: no point inside the mover's swept volume that the oracle labels dynamic, before or after; and every point
    # of it is a world point of a point the report kept
    lo, hi = _center(0) - HALF - 0.15, _center(9) + HALF + 0.15
    for name, x in (("colored_after", on["poses"]), ("colored_before", args[1])):
        world = np.concatenate([do.world_points(c, T) for c, T in zip(clouds, np.asarray(x).reshape(-1, 12))]).astype(np.float32)
        inside = ((world >= lo) & (world <= hi)).all(1)
        if name == "colored_after":
            assert inside[mover].mean() > 0.99 and not inside[~mover].any()
            assert int((ref["label"][inside] != 0).sum()) > 0.5 * mover.sum()              # the oracle labels most of the mover
        gone = _rows(world[inside & (ref["label"] != 0)])
        got = _rows(on[name][0])
        assert len(got) > 1000 and not np.isin(gone, got).any(), name
        kept = _rows(world[rep["label"] == 0])
        assert np.isin(got, kept).all(), name
        had = int(np.isin(gone, _rows(plain[name][0])).sum())
        print(f"{name}: {len(got)} points; of the {len(gone)} oracle-dynamic points in the swept volume the plain run's map holds {had}")


def test_run_dataset_writes_the_dynamic_report(pkg, tmp_path):
    """The same sequence through the on-disk formats (as tests/test_gpu_pipeline.py writes them): run_dataset(remove_dynamic=...)
    returns the report and writes dynamic.json -- the summary and the per-frame counts -- beside map_quality.json; without the
    option neither the key nor the file appears."""
    import json
    import sqlite3
    import test_gpu_pipeline as tp
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    args, cfg, _, clouds, mover = _dataset()
    _, odo, times, img_t, _, _, _, _, _, _, kps, pairs, matches = args
    root = tmp_path / "seq"
    (root / "all_pcd_body").mkdir(parents=True); (root / "all_image").mkdir()
    for t, c in zip(times, clouds):
        ds.save_pcd(str(root / "all_pcd_body" / f"{t:.6f}.pcd"), np.concatenate([c, np.zeros((len(c), 1), np.float32)], 1))
    ds.write_poses_tum(str(root / "all_pcd_body" / "lidar_poses.txt"), times, odo)
    for t in img_t:
        (root / "all_image" / f"{t:.6f}.png").write_bytes(b"")
    ds.write_poses_tum(str(root / "all_image" / "image_poses.txt"), img_t, odo)
    con = sqlite3.connect(str(root / "colmap.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    for i, t in enumerate(img_t):
        kp4 = np.concatenate([kps[i], np.ones((len(kps[i]), 2), np.float32)], 1).astype(np.float32)
        con.execute("INSERT INTO images VALUES (?, ?)", (i + 1, f"{t:.6f}.png"))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (i + 1, kp4.shape[0], 4, kp4.tobytes()))
    for (i, j), m in zip(pairs, matches):
        con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                    (ds.image_ids_to_pair_id(i + 1, j + 1), len(m), 2, np.asarray(m, np.uint32).tobytes()))
    con.commit(); con.close()
    opts = dict(window=4, min_free=2)
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(tmp_path / "on"),
                           remove_dynamic=opts, map_quality=dict(query_stride=2001), **cfg)
    rep = got["dynamic"]
    with pkg.Scans(clouds) as sc:
        static, direct = pipe.remove_dynamic(sc, got["poses"], **opts)
        static.close()
    assert direct["label"].tobytes() == rep["label"].tobytes() and rep["n_dynamic"] > 0.5 * mover.sum()
    saved = json.loads((tmp_path / "on" / "dynamic.json").read_text())
    assert sorted(saved) == ["ms", "n_dynamic", "n_judged", "n_points", "per_frame"]
    assert [saved[k] for k in ("n_points", "n_judged", "n_dynamic")] == [rep[k] for k in ("n_points", "n_judged", "n_dynamic")]
    assert saved["per_frame"] == [int(x) for x in rep["per_frame"]] and sum(saved["per_frame"]) == rep["n_dynamic"]
    assert (tmp_path / "on" / "map_quality.json").exists()
    assert got["map_quality"]["after"]["n_points"] == rep["n_points"] - rep["n_dynamic"]
    off = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(tmp_path / "off"), **cfg)
    assert "dynamic" not in off and not (tmp_path / "off" / "dynamic.json").exists()
    assert np.abs(off["poses"] - got["poses"]).max() == 0.0
