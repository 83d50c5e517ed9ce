"""CPU tests of the LiDAR stage's pose priors: the numpy model (tests/prior_oracle.py) against central finite differences, the
device header csrc/prior_device.h compiled for the host against the model, and the C-ABI / Python surface."""
import math
import os
import subprocess

import numpy as np
import pytest

import prior_oracle as po
from conftest import ROOT

KINDS = ["pose", "position", "relative"]


def _rand_rot(rng, angle=None):
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    return po.so3_exp(w * (rng.uniform(0.1, 3.0) if angle is None else angle))


def _pose(R, p):
    return np.r_[np.asarray(R).reshape(9), np.asarray(p).reshape(3)]


def _case(rng, kind, offsets, regime):
    """(prior, poses [2, 12]): pose 0 = i, pose 1 = j; the rotation residual near 0 ('ident'), near pi ('pi') or anywhere"""
    Ti = _pose(_rand_rot(rng), rng.normal(scale=5.0, size=3))
    Tj = _pose(_rand_rot(rng), rng.normal(scale=5.0, size=3))
    oi = _pose(_rand_rot(rng), rng.normal(size=3)) if offsets else po.IDENT
    oj = _pose(_rand_rot(rng), rng.normal(size=3)) if offsets else po.IDENT
    A = po.compose(Ti, oi)
    B = po.compose(Tj, oj)
    R_true = A[0] if kind != "relative" else A[0].T @ B[0]
    ang = {"ident": 1e-3, "pi": math.pi - 1e-3, "any": None}[regime]
    Rm = R_true @ _rand_rot(rng, ang).T
    meas = _pose(Rm, rng.normal(size=3))
    L = np.tril(rng.normal(size=(6, 6))) + 3.0 * np.eye(6)
    pr = po.make_prior(kind, 0, meas, L, j=1 if kind == "relative" else 0, oi=oi, oj=oj)
    return pr, np.stack([Ti, Tj])


CASES = [(k, off, reg) for k in KINDS for off in (False, True) for reg in ("ident", "pi", "any")]


@pytest.mark.parametrize("kind,offsets,regime", CASES)
def test_oracle_jacobians_match_central_differences(kind, offsets, regime):
    rng = np.random.default_rng(hash((kind, offsets, regime)) % 2**32)
    for _ in range(3):
        pr, x = _case(rng, kind, offsets, regime)
        r, Ji, Jj = po.raw(pr, x[0], x[1])
        if regime == "pi" and kind != "position":
            assert abs(np.linalg.norm(r[:3]) - math.pi) < 2e-3
        h = 1e-6
        for pose, J in ((0, Ji), (1, Jj)):
            num = np.zeros((6, 6))
            for c in range(6):
                d = np.zeros((2, 6))
                d[pose, c] = h
                rp, _, _ = po.raw(pr, *po.retract(x, d.reshape(-1)))
                rm, _, _ = po.raw(pr, *po.retract(x, -d.reshape(-1)))
                num[:, c] = (rp - rm) / (2 * h)
            if pose == 1 and kind != "relative":
                assert not J.any()
            assert np.abs(num - J).max() <= 1e-6 * max(1.0, np.abs(J).max()), (kind, pose, num - J)


def test_log_exp_round_trip_near_zero_and_pi():
    rng = np.random.default_rng(3)
    for ang in (1e-12, 1e-7, 1e-4, 0.3, 2.0, math.pi - 1e-4, math.pi - 1e-8):
        for _ in range(5):
            w = rng.normal(size=3)
            w *= ang / np.linalg.norm(w)
            back = po.so3_log(po.so3_exp(w))
            assert np.abs(back - w).max() <= 1e-12 * max(1.0, ang) + 1e-15, (ang, back - w)


def _checker(tmp_path):
    exe = str(tmp_path / "prior_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "prior_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """[(prior, poses, the checker's output line as doubles)] of the cases, four draws each"""
    exe = _checker(tmp_path_factory.mktemp("prior_check"))
    rng = np.random.default_rng(11)
    lines, cases = [], []
    for kind, off, reg in CASES * 4:
        pr, x = _case(rng, kind, off, reg)
        cases.append((pr, x))
        vals = np.r_[x[0], x[1], pr["oi"], pr["oj"], pr["meas"], pr["L"].reshape(-1)]
        lines.append(f"{pr['kind']} " + " ".join(float(v).hex() for v in vals))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [(pr, x, np.array([float.fromhex(t) for t in ln.split()])) for (pr, x), ln in zip(cases, out)]
    assert len(got) == len(cases) and all(v.size == 6 + 6 + 36 + 36 + 1 + 2 * 128 for _, _, v in got)
    return got


def test_device_header_agrees_with_the_oracle(checked):
    """csrc/prior_device.h (host build) vs the numpy model: residual, whitened residual, whitened Jacobians and cost agree to a
    few ulp of each quantity's scale (the two sum the same products in different orders)."""
    eps = np.finfo(np.float64).eps
    for pr, x, v in checked:
        r, Ji, Jj = po.raw(pr, x[0], x[1])
        e, Wi, Wj = po.whiten(pr, r, Ji, Jj)
        for got, ref in ((v[:6], r), (v[6:12], e), (v[12:48], Wi.reshape(-1)), (v[48:84], Wj.reshape(-1)), (v[84:85], [0.5 * e @ e])):
            ref = np.asarray(ref)
            scale = max(np.abs(ref).max(), 1e-300)
            assert np.abs(got - ref).max() <= 64 * eps * scale, (pr["kind"], got - ref)


def _close(a, b, what):
    """tests/test_posegraph_host.py's tolerance for a lin record against its oracle"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max(initial=0.0)))
    assert np.abs(a - b).max(initial=0.0) <= 1e-12 * scale, what


def test_lin_record_holds_the_products_of_the_whitened_blocks(checked):
    """prior_eval + prior_record (what prior_lin_kernel runs per prior), all three kinds: the record's W^T e and W^T W against numpy's
    from the same program's e, W_i, W_j, the cross block in both orientations; what a POSE / POSITION record does not own -- the
    j ranges, the cross block -- and the unused slots keep the sentinel the checker pre-filled."""
    SENTINEL = -777.0
    seen = set()
    for pr, x, v in checked:
        e, Wi, Wj = v[6:12], v[12:48].reshape(6, 6), v[48:84].reshape(6, 6)
        seen.add(pr["kind"])
        for flip in (0, 1):
            o = v[85 + 128 * flip:85 + 128 * (flip + 1)]
            what = (pr["kind"], flip)
            _close(o[1:7], Wi.T @ e, what)
            _close(o[13:49].reshape(6, 6).T, Wi.T @ Wi, what)
            assert o[0] == SENTINEL and (o[121:] == SENTINEL).all(), what
            if pr["kind"] == po.KINDS["relative"]:
                _close(o[7:13], Wj.T @ e, what)
                _close(o[49:85].reshape(6, 6).T, Wj.T @ Wj, what)
                X = Wi.T @ Wj
                _close(o[85:121].reshape(6, 6).T, X.T if flip else X, what)
            else:
                assert (o[7:13] == SENTINEL).all() and (o[49:121] == SENTINEL).all(), what
        if pr["kind"] == po.KINDS["position"]:          # rows 3..5 of a POSITION block are zero: nothing of L beyond 3 x 3 enters
            assert not Wi[3:].any() and not e[3:].any()
    assert seen == set(po.KINDS.values())


def test_prior_struct_and_kinds_match_the_c_header(pkg, tmp_path):
    L = pkg._lib
    src = tmp_path / "prior.c"
    src.write_text('#include <stdio.h>\n#include "lvba_hip.h"\n'
                   'int main(void){printf("%d %d %d\\n", LVBA_PRIOR_POSE, LVBA_PRIOR_POSITION, LVBA_PRIOR_RELATIVE); return 0;}\n')
    exe = str(tmp_path / "prior")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v == [L.PRIOR_KINDS[k] for k in KINDS] == [po.KINDS[k] for k in KINDS]      # lvba_prior's layout: tests/test_abi.py
    assert {"lvba_balm_set_priors", "lvba_balm_prior_residuals"} <= set(L.SYMBOLS)


def test_python_prior_helpers(pkg):
    P = pkg.Prior
    R = po.so3_exp([0.1, -0.2, 0.3])
    a = P.pose(3, (R, [1.0, 2.0, 3.0]), sigma_rot=0.01, sigma_pos=[0.1, 0.2, 0.5])
    assert a.kind == 0 and a.i == 3 and np.allclose(np.array(a.meas[:9]).reshape(3, 3), R) and list(a.meas[9:]) == [1.0, 2.0, 3.0]
    assert np.allclose(np.array(a.sqrt_info).reshape(6, 6), np.diag([100, 100, 100, 10, 5, 2]))
    assert not any(a.offset_i)                       # identity by default (twelve zeros)
    b = P.position(7, [4.0, 5.0, 6.0], sigma=0.05, lever_arm=[0.0, 0.0, 1.5])
    assert b.kind == 1 and list(b.meas[9:]) == [4.0, 5.0, 6.0] and list(b.offset_i[9:]) == [0.0, 0.0, 1.5]
    assert np.allclose(np.array(b.sqrt_info).reshape(6, 6)[:3, :3], 20.0 * np.eye(3)) and not np.array(b.sqrt_info).reshape(6, 6)[3:].any()
    T = np.eye(4)
    T[:3, 3] = [1.0, 0.0, 0.0]
    c = P.relative(0, 9, T, sqrt_info=2.0 * np.eye(6))
    assert c.kind == 2 and (c.i, c.j) == (0, 9) and c.meas[9] == 1.0 and c.sqrt_info[0] == 2.0
    with pytest.raises(ValueError):
        P.pose(0, T)


def test_cpp_adapter_prior_helpers_compile_and_pack(pkg, tmp_path):
    """include/lvba_adapter.hpp: prior_pose / prior_position / prior_relative and the overloads that take priors (stand-in types);
    without a device the library refuses loudly."""
    import __graft_entry__ as ge
    ge.build()
    exe = str(tmp_path / "adapter_priors_check")
    libdir = os.path.join(ROOT, "global-lvba_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "adapter_priors_check.cpp"), "-o", exe,
                           "-L", libdir, "-llvba_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_pipeline_passes_lidar_priors_on(pkg, monkeypatch):
    """run_full_pipeline(lidar_priors=...) hands the priors to Scans.lidar_ba"""
    import importlib
    pl = importlib.import_module("global-lvba_amd.pipeline")
    seen = {}

    class FakeScans:
        def __init__(self, clouds, device=0):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def lidar_ba(self, x, priors=None, **kw):
            seen["priors"] = priors
            return x, {}

    monkeypatch.setattr(pl, "Scans", FakeScans)
    fix = [pkg.Prior.position(0, [0.0, 0.0, 0.0], sigma=0.1)]
    out = pl.run_full_pipeline([np.zeros((1, 3), np.float32)], np.r_[np.eye(3).reshape(9), 0, 0, 0][None], [0.0], [], None, None,
                               None, None, 1, 1, None, None, None, enable_visual_ba=False, lidar_priors=fix)
    assert seen["priors"] is fix and out["poses"].shape == (1, 12)
