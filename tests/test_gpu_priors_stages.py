"""GPU tests of pose priors on FRAMES in the global stages of the LiDAR BA (lvba_lidar_ba_priors / lvba_lidar_ba_multi_priors,
Scans.lidar_ba(priors=...)) and of the C++ adapter's prior helpers."""
import os
import subprocess

import numpy as np
import pytest

import prior_oracle as po
from conftest import ROOT

pytestmark = pytest.mark.gpu

KW = dict(window_size=4, anchor_leaf=0.05, stage_voxel_size=(1.0, 0.5))


def _scene(synth, n=12, seed=41):
    return synth.make_scans(n, 8000, room=(10, 8, 4), origin=(-3.3, 7.1, 0.4), n_panels=8, seed=seed, rot_sigma_deg=0.1,
                            trans_sigma=0.03)


def _compose(A, B):
    A, B = np.asarray(A).reshape(12), np.asarray(B).reshape(12)
    RA, RB = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    return np.r_[(RA @ RB).reshape(9), RA @ B[9:] + A[9:]]


def _as_dict(p):
    return dict(kind=p.kind, i=p.i, j=p.j, meas=np.array(p.meas[:]), L=np.array(p.sqrt_info[:]).reshape(6, 6),
                oi=np.array(p.offset_i[:]) if any(p.offset_i) else po.IDENT.copy(),
                oj=np.array(p.offset_j[:]) if any(p.offset_j) else po.IDENT.copy())


@pytest.mark.parametrize("window_enable", [True, False])
def test_zero_priors_change_no_byte(pkg, synth, window_enable):
    s = _scene(synth)
    with pkg.Scans(s["clouds"]) as sc:
        a, ra = sc.lidar_ba(s["poses"], window_enable=window_enable, **KW)
        b, rb = sc.lidar_ba(s["poses"], window_enable=window_enable, priors=[], **KW)
    assert a.tobytes() == b.tobytes() and rb["priors_used"] == rb["priors_dropped"] == 0
    assert ra["stage_cost_last"] == rb["stage_cost_last"]
    s2 = _scene(synth, 16, 43)
    m1, _ = pkg.Scans.lidar_ba_multi(s2["clouds"], s2["poses"], (0, 0), **KW)
    m2, _ = pkg.Scans.lidar_ba_multi(s2["clouds"], s2["poses"], (0, 0), priors=[], **KW)
    assert m1.tobytes() == m2.tobytes()


def test_frame_position_priors_pull_to_the_truth(pkg, synth):
    s = _scene(synth)
    gt = s["poses_gt"].reshape(-1, 12)
    x0 = s["poses"].reshape(-1, 12).copy()
    x0[:, 9:] += np.array([0.4, -0.3, 0.2])                     # a planted offset: the voxel cost cannot see it
    arm = np.array([0.1, 0.0, 0.3])
    fixes = [pkg.Prior.position(f, gt[f, :9].reshape(3, 3) @ arm + gt[f, 9:], sigma=0.01, lever_arm=arm) for f in range(len(gt))]

    def rmse(x):
        return float(np.sqrt(((x[:, 9:] - gt[:, 9:]) ** 2).sum(1).mean()))

    with pkg.Scans(s["clouds"]) as sc:
        free, _ = sc.lidar_ba(x0, **KW)
        got, rep = sc.lidar_ba(x0, priors=fixes, **KW)
    assert rep["priors_used"] + rep["priors_dropped"] == len(fixes) and rep["priors_used"] >= len(fixes) - 4 * rep["n_windows_skipped"]
    assert rmse(got) < 0.5 * rmse(free) and rmse(got) < 0.1


def test_frame_priors_map_exactly_onto_the_anchors(pkg, synth):
    """a frame f of anchor a with rel_f becomes a prior on a with offset rel_f o O: its residual at the anchor pose equals the frame
    prior's residual at anchor o rel_f; relative priors inside one anchor are dropped"""
    s = _scene(synth)
    x = s["poses"].reshape(-1, 12)
    arm = np.r_[po.so3_exp([0.1, -0.2, 0.05]).reshape(9), 0.3, 0.1, -0.2]
    P = pkg.Prior
    frame = [P.position(1, x[1, 9:], sigma=0.05, lever_arm=[0.0, 0.0, 1.0]),
             P.pose(6, x[6], sigma_rot=0.01, sigma_pos=0.05, offset=arm),
             P.relative(2, 9, _compose(np.r_[x[2, :9].reshape(3, 3).T.reshape(9), -x[2, :9].reshape(3, 3).T @ x[2, 9:]], x[9]),
                        sigma_rot=0.01, sigma_pos=0.05, offset_i=arm, offset_j=arm),
             P.relative(4, 5, np.eye(4), sigma_rot=0.01, sigma_pos=0.05)]           # frames 4 and 5: one window, one anchor
    with pkg.Scans(s["clouds"]) as sc:
        wb = sc.window_ba(x, window_size=KW["window_size"], voxel_size=KW["stage_voxel_size"][0], anchor_leaf=KW["anchor_leaf"])
        wb["anchor_scans"].close()
        _, rep = sc.lidar_ba(x, priors=frame, **KW)
    aidx, rel, A = wb["anchor_index"], wb["rel_poses"], wb["anchor_poses"]
    assert rep["n_windows_skipped"] == 0 and rep["priors_used"] == 3 and rep["priors_dropped"] == 1
    for fp, ap in zip(frame[:3], rep["anchor_priors"]):
        f, a = _as_dict(fp), _as_dict(ap)
        assert a["i"] == aidx[f["i"]] and (f["kind"] != 2 or a["j"] == aidx[f["j"]])
        assert np.abs(a["oi"] - _compose(rel[f["i"]], f["oi"])).max() <= 1e-15 * 10
        frames = np.stack([_compose(A[aidx[k]], rel[k]) for k in range(len(x))])
        e_f, c_f = po.residual(f, frames)
        e_a, c_a = po.residual(a, A)
        assert np.abs(e_a - e_f).max() <= 1e-9 * max(1.0, np.abs(e_f).max()) and abs(c_a - c_f) <= 1e-9 * max(c_f, 1e-12)


def test_cpp_adapter_refines_with_priors(tmp_path):
    exe = str(tmp_path / "adapter_priors_check")
    libdir = os.path.join(ROOT, "global-lvba_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "adapter_priors_check.cpp"), "-o", exe,
                           "-L", libdir, "-llvba_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refined on the GPU with priors" in out.stdout and "lidar_ba with frame priors on the GPU" in out.stdout
