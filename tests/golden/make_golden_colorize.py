"""Generates tests/golden/ref_colorize.npz: the reference's own LvbaSystem::VisualizeOptComparison (src/lvba_system.cpp:1932-2144,
compiled from the reference sources against oracle/shim: oracle/_ref/liblvba_system_ref.so) on the synthetic sequence of
tests/test_ref_system.py after runLidarBA, so that the refined and the original poses differ.  The stand-in cv::imread hands
out the pattern (b, g, r) = (x, y, x + y) mod 256.  Stored: the sorted rows of points3D.txt without their index, the scan and
camera poses the reference used, the scan and image times, and a digest of the clouds, so that tests/test_gpu_colorize.py
(where the reference does not exist) regenerates the same inputs, checks them, and holds the device against the rows.

    python tests/golden/make_golden_colorize.py
"""
import hashlib
import importlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))

SEQ = dict(n_frames=12, pts=3000, n_land=260, seed=63)


def clouds_digest(clouds):
    h = hashlib.sha256()
    for c in clouds:
        h.update(np.ascontiguousarray(np.asarray(c, np.float32)[:, :3]).tobytes())
    return h.hexdigest()


def sequence():
    import test_gpu_pipeline as tp
    import test_ref_system as trs
    return tp._dataset(INTR=trs.INTR, W=trs.W, H=trs.H, **SEQ)


def reference_run(root, d):
    """Writes the sequence under root, runs the reference up to VisualizeOptComparison; returns the fixture's arrays."""
    import test_gpu_pipeline as tp
    import test_ref_system as trs
    from oracle import ref_system as rs
    ds = importlib.import_module("global-lvba_amd.dataset")
    trs.write_sequence(root, d, ds)
    S = rs.ReferenceSystem(root, trs.reference_params(tp))
    try:
        S.init()
        S.run_lidar_ba()
        S.build_grid_map(); S.update_camera_poses(); S.generate_depth(trs.W, trs.H)
        R1, p1, ts = S.scan_poses()
        R0, p0, _ = S.scan_poses(before=True)
        Rc1, tc1 = S.cam_poses(True)
        Rc0, tc0 = S.cam_poses(False)
        clouds = [S.cloud(i)[:, :3].copy() for i in range(S.n_clouds)]
        ids = S.image_ids()
        S.export_colmap(trs.W, trs.H)
    finally:
        S.close()
    rows = open(os.path.join(root, "Colmap", "sparse", "points3D.txt")).read().splitlines()
    rows = sorted(" ".join(r.split()[1:]) for r in rows)
    return dict(rows="\n".join(rows), n_rows=len(rows), scan_after=np.concatenate([R1.reshape(-1, 9), p1], 1),
                scan_before=np.concatenate([R0.reshape(-1, 9), p0], 1), scan_times=ts, Rcw_after=Rc1, tcw_after=tc1,
                Rcw_before=Rc0, tcw_before=tc0, image_times=ids, intr=trs.INTR, width=trs.W, height=trs.H,
                clouds_sha256=clouds_digest(clouds), clouds=clouds)


def main():
    d = sequence()
    with tempfile.TemporaryDirectory() as tmp:
        r = reference_run(os.path.join(tmp, "seq"), d)
    assert r["clouds_sha256"] == clouds_digest(d["clouds"])
    r.pop("clouds")
    np.savez_compressed(os.path.join(HERE, "ref_colorize.npz"), seq=np.array([SEQ[k] for k in ("n_frames", "pts", "n_land", "seed")]),
                        **r)
    print(f"ref_colorize.npz: {r['n_rows']} points3D rows")


if __name__ == "__main__":
    main()
