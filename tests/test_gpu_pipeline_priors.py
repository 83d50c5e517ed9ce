"""Camera pose priors through the host-side pipeline mirror: tests/test_gpu_pipeline.py's synthetic sequence through
run_full_pipeline(camera_priors=lambda cams: lidar_camera_priors(cams, ...))."""
import importlib

import numpy as np
import pytest

import visual_prior_oracle as vpo
from test_gpu_pipeline import H, INTR, RCB, TCI, W, _dataset

pytestmark = pytest.mark.gpu

# "Tight": far stronger than what the images say about a camera.  A camera with ~100 observations at f = 300 px, depth ~5 m and
# sigma_px = 0.5 carries at most I_v ~ 100 (300 / (5 * 0.5))^2 ~ 1e6 / m^2 of position information (landmarks held fixed; less
# with free landmarks), and the free visual stage moves it by d < 0.1 m (tests/test_gpu_pipeline.py).  With a prior of sigma the
# minimum sits at d I_v / (I_v + 1 / sigma^2) from the prior, i.e. d I_v sigma / (I_v sigma^2 + 1) sigmas: < 2 for
# sigma = 2e-5 m.  The same count for the rotation (I_v ~ 100 (300 / 0.5)^2 ~ 4e7 / rad^2, d ~ 3e-3 rad) gives 0.2 sigmas at 2e-6.
TIGHT_ROT, TIGHT_POS = 2e-6, 2e-5


def _run(pipe, d, camera_priors=None):
    return pipe.run_full_pipeline(d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], RCB, TCI, INTR, W, H, d["kps"], d["pairs"],
                                  d["matches"], window_size=6, anchor_leaf=0.02, stage_voxel_size=(1.0, 0.5),
                                  stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4), camera_priors=camera_priors)["visual"]


def test_pipeline_camera_priors(pkg):
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    d = _dataset()
    free = _run(pipe, d)
    seen = []

    def loose(cams):
        seen.append(np.array(cams))
        return pipe.lidar_camera_priors(cams, RCB, TCI, 1e6, 1e6)

    v = _run(pipe, d, loose)
    assert len(seen) == 1 and np.array_equal(seen[0], v["cam_poses"]) and np.array_equal(v["cam_poses"], free["cam_poses"])
    print("sigma 1e6: cameras differ by", np.abs(v["Rcw"] - free["Rcw"]).max(), np.abs(v["tcw"] - free["tcw"]).max())
    assert np.abs(v["Rcw"] - free["Rcw"]).max() <= 1e-7 and np.abs(v["tcw"] - free["tcw"]).max() <= 1e-7
    # tight priors: every whitened prior residual component of the refined cameras is within 3 (sigmas)
    tight = _run(pipe, d, lambda cams: pipe.lidar_camera_priors(cams, RCB, TCI, TIGHT_ROT, TIGHT_POS))
    priors = pipe.lidar_camera_priors(tight["cam_poses"], RCB, TCI, TIGHT_ROT, TIGHT_POS)
    # at the LiDAR-derived cameras the visual stage starts from, the priors' residuals vanish: measurement, extrinsic offset and
    # the cameras of camera_from_imu state the same poses (sigma 2e-5 m: 1e-3 is 2e-8 m)
    q_start = pipe.rot_to_quat_wxyz(tight["Rcw_lidar"])
    e_start = np.array([vpo.prior_block(p, q_start, tight["tcw_lidar"], False)[0] for p in priors])
    print("prior residuals at the starting cameras (sigmas)", np.abs(e_start).max())
    assert np.abs(e_start).max() <= 1e-3
    e = np.array([vpo.prior_block(p, tight["q"], tight["tcw"], False)[0] for p in priors])
    e_free = np.array([vpo.prior_block(p, free["q"], free["tcw"], False)[0] for p in priors])
    print("tight: largest |e| (sigmas)", np.abs(e).max(), "without priors", np.abs(e_free).max())
    assert tight["termination"].startswith("CONVERGENCE")
    assert np.abs(e).max() <= 3.0
    assert np.abs(e_free).max() > 3.0                                    # the free run does leave the LiDAR-derived cameras
    # relative priors run as well and keep the trajectory's shape closer to the LiDAR's than the free run
    rel = _run(pipe, d, lambda cams: pipe.lidar_camera_priors(cams, RCB, TCI, TIGHT_ROT, TIGHT_POS, relative=True))
    pr = pipe.lidar_camera_priors(rel["cam_poses"], RCB, TCI, TIGHT_ROT, TIGHT_POS, relative=True)
    er = np.array([vpo.prior_block(p, rel["q"], rel["tcw"], False)[0] for p in pr])
    er_free = np.array([vpo.prior_block(p, free["q"], free["tcw"], False)[0] for p in pr])
    print("relative: largest |e|", np.abs(er).max(), "without priors", np.abs(er_free).max())
    assert np.abs(er).max() < np.abs(er_free).max()
