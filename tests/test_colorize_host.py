"""CPU tests of the LiDAR map colouriser (lvba_colorize_*): the restatement (tests/colorize_oracle.py) pinned to the reference's
own VisualizeOptComparison, the device header (csrc/colorize_device.h) compiled for the host against a literal sequential
walk and the restatement, and the Python layer around it (image decoding, the PCD XYZRGB writer, run_dataset's default)."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from host_build import build_check

import colorize_oracle as co

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


# ---------------------------------------------------------------------------------------------------------------- (a) reference
def test_oracle_matches_reference_visualize_opt_comparison(tmp_path):
    """The sequence of test_ref_system.py after runLidarBA: the reference's points3D.txt (its after-cloud, thinned at 0.01 m)
    against the restatement, line for line as sorted multisets; the before-cloud differs."""
    from oracle import ref_system as rs
    if not rs.available():
        pytest.skip("no reference sources and no prebuilt oracle/_ref/liblvba_system_ref.so")
    import make_golden_colorize as mg
    d = mg.sequence()
    r = mg.reference_run(str(tmp_path / "seq"), d)
    img = co.pattern_image(int(r["width"]), int(r["height"]))
    args = (r["clouds"], r["scan_times"], r["image_times"])
    xyz, rgb = co.colorize(r["clouds"], r["scan_after"], r["scan_times"], r["image_times"], r["Rcw_after"], r["tcw_after"],
                           r["intr"], int(r["width"]), int(r["height"]), lambda k: img)
    rows = r["rows"].split("\n")
    assert len(rows) == r["n_rows"] > 5000
    assert sorted(co.points3d_lines(xyz, rgb)) == rows
    xb, cb = co.colorize(*args[:1], r["scan_before"], *args[1:], r["Rcw_before"], r["tcw_before"], r["intr"], int(r["width"]),
                         int(r["height"]), lambda k: img)
    assert sorted(co.points3d_lines(xb, cb)) != rows
    # the stored fixture is this very run (the GPU tests read it)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_colorize.npz"))
    assert str(g["rows"]) == r["rows"] and str(g["clouds_sha256"]) == r["clouds_sha256"]
    assert np.array_equal(g["scan_after"], r["scan_after"]) and np.array_equal(g["Rcw_before"], r["Rcw_before"])


# ------------------------------------------------------------------------------------------------------- (b) host-built header
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("colorize_check", tmp_path_factory.mktemp("emul_colorize")))
    f64 = np.ctypeslib.ndpointer(np.float64, flags="C")
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    i64 = np.ctypeslib.ndpointer(np.int64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
    c64 = ctypes.c_int64
    lib.emul_walks.argtypes = [c64, i64, f64, u8, i64]
    lib.emul_project.argtypes = [c64, f32, f64, f64, f64, ctypes.c_int, ctypes.c_int, u8, i64, f64]
    lib.emul_world.argtypes = [c64, f32, f64, f32]
    lib.emul_leaf_key.argtypes = [c64, f32, ctypes.c_double, i64, f64, u8]
    lib.emul_window.argtypes = [ctypes.c_int, f64, ctypes.c_double, ctypes.c_double, i32, u8]
    return lib


def literal_walk(zcs):
    """The reference's loop over one pixel written out with a float32 buffer (src/lvba_system.cpp:2046-2058)."""
    zbuf = np.float32(np.inf)
    win = -1
    for q, zc in enumerate(zcs):
        if float(zc) + float(np.float32(1e-6)) < float(zbuf):
            zbuf = np.float32(zc)
            win = q
    return (win >= 0 and bool(np.isfinite(zbuf))), win


def adversarial_runs(rng, n_runs):
    """Pixel runs built to break a minimum-depth shortcut: exact duplicates, depths within 1e-6, far depths (17-300 m, where
    one float ulp exceeds 1e-6), ascending / descending chains one ulp apart, NaN and negative depths."""
    runs = []
    for r in range(n_runs):
        kind = r % 6
        n = int(rng.integers(1, 12))
        base = float(rng.choice([rng.uniform(0.1, 5.0), rng.uniform(17.0, 300.0)]))
        if kind == 0:
            z = np.full(n, base)
        elif kind == 1:
            z = base + rng.uniform(-1.5e-6, 1.5e-6, n)
        elif kind == 2:
            ulp = float(np.spacing(np.float32(base)))
            z = base + ulp * rng.integers(-3, 4, n) + rng.uniform(-1e-6, 1e-6, n)
        elif kind == 3:
            z = base - np.arange(n) * rng.choice([4e-7, 1e-6, 1.1e-6, float(np.spacing(np.float32(base)))])
        elif kind == 4:
            z = base + rng.uniform(-1e-3, 1e-3, n)
            z[rng.random(n) < 0.3] = np.nan
            z[rng.random(n) < 0.2] *= -1
        else:
            z = np.float32(base + rng.uniform(-2e-5, 2e-5, n)).astype(np.float64) + rng.choice([0.0, 5e-7, 1e-6], n)
        runs.append(np.asarray(z, np.float64))
    return runs


def test_device_walk_equals_literal_walk(emul):
    rng = np.random.default_rng(11)
    runs = adversarial_runs(rng, 120000)
    off = np.concatenate([[0], np.cumsum([len(z) for z in runs])]).astype(np.int64)
    zc = np.concatenate(runs)
    kept, win = np.zeros(len(runs), np.uint8), np.zeros(len(runs), np.int64)
    emul.emul_walks(len(runs), off, zc, kept, win)
    n_not_min = 0
    for s, z in enumerate(runs):
        k, w = literal_walk(z)
        assert (bool(kept[s]), int(win[s]) if k else -1) == (k, w if k else -1), (s, z)
        assert co.depth_walk(z.tolist()) == (k, w) or not k
        with np.errstate(invalid="ignore"):
            fin = np.where(np.isfinite(z), z, np.inf)
        n_not_min += k and w != int(np.argmin(fin))
    assert n_not_min > 1000                                  # the rule is not "minimum depth, first on ties"


def test_device_projection_and_world_points_match_restatement(emul):
    rng = np.random.default_rng(5)
    W, H = 64, 48
    intr = np.array([50.0, 49.0, 31.7, 23.2, -0.07, 0.12, -0.001, 0.0003])
    R = np.eye(3)
    t = np.zeros(3)
    n = 60000
    Z = rng.choice([rng.uniform(0.5, 20.0), -1.0], n).astype(np.float64) * rng.uniform(0.5, 1.5, n)
    # pixel edges: points that land within 1e-9 of a half-integer u or v
    u = rng.integers(-2, W + 2, n) + 0.5 + rng.choice([0.0, 1e-12, -1e-12, 0.25], n)
    v = rng.integers(-2, H + 2, n) + 0.5 + rng.choice([0.0, 1e-12, -1e-12, 0.25], n)
    X = np.stack([(u - intr[2]) / intr[0] * Z, (v - intr[3]) / intr[1] * Z, Z], 1)
    X[rng.random(n) < 0.02] = np.nan
    pw = X.astype(np.float32)
    ok, pix, zc = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n)
    emul.emul_project(n, pw, R.reshape(-1).copy(), t, intr, W, H, ok, pix, zc)
    ok2, pix2, zc2 = co.project(pw, R, t, intr, W, H)
    assert np.array_equal(ok.astype(bool), ok2) and ok2.sum() > 10000
    assert np.array_equal(pix[ok2], pix2[ok2]) and np.array_equal(zc[ok2], zc2[ok2])
    T = np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0].reshape(-1), rng.uniform(-50, 50, 3)])
    cloud = rng.uniform(-80, 80, (n, 3)).astype(np.float32)
    out = np.zeros((n, 3), np.float32)
    emul.emul_world(n, cloud, T, out)
    assert np.array_equal(out, co.world_points(cloud, T))


def test_device_leaf_key_matches_restatement(emul):
    rng = np.random.default_rng(9)
    n = 100000
    xyz = np.concatenate([rng.uniform(-30, 30, (n // 2, 3)), np.round(rng.uniform(-3, 3, (n // 2, 3)), 2)]).astype(np.float32)
    for leaf in (0.01, 0.05, 0.2):
        k, d2, ok = np.zeros((n, 3), np.int64), np.zeros(n), np.zeros(n, np.uint8)
        emul.emul_leaf_key(n, xyz, leaf, k, d2, ok)
        k2, d22 = co.leaf_keys(xyz, leaf)
        assert ok.all() and np.array_equal(k, k2) and np.array_equal(d2, d22)
    far = np.array([[2.0e4, 0, 0], [np.nan, 0, 0]], np.float32)
    k, d2, ok = np.zeros((2, 3), np.int64), np.zeros(2), np.zeros(2, np.uint8)
    emul.emul_leaf_key(2, far, 0.01, k, d2, ok)
    assert not ok.any()


def test_device_window_matches_reference_rule(emul):
    rng = np.random.default_rng(3)
    for _ in range(2000):
        t = np.sort(50.0 + np.round(rng.uniform(0, 3, int(rng.integers(1, 40))), int(rng.integers(1, 4))))
        ti = float(rng.choice(t) + rng.choice([0.5, -0.5, 0.0, 0.004, 0.5 + 1e-12]))
        lohi, inside = np.zeros(2, np.int32), np.zeros(len(t), np.uint8)
        emul.emul_window(len(t), t, ti, 0.5, lohi, inside)
        ref = np.array([not abs(x - ti) > 0.5 for x in t])
        assert np.array_equal(inside.astype(bool), ref)
        rng_ = np.zeros(len(t), bool)
        rng_[lohi[0]:lohi[1]] = True
        assert np.array_equal(rng_, ref)


def test_oracle_thinning_keeps_first_minimum_in_merged_order():
    xyz = np.array([[0.005, 0.005, 0.005], [0.004, 0.005, 0.005], [0.005, 0.005, 0.005], [0.006, 0.005, 0.005],
                    [-0.005, 0.005, 0.005]], np.float32)
    rgb = np.arange(15, dtype=np.uint8).reshape(5, 3)
    x, c = co.down_sampling_voxel2(xyz, rgb, 0.01)
    assert len(x) == 2 and np.array_equal(c, rgb[[4, 0]])   # the same d2 at merged positions 0 and 2: position 0 wins
    x, c = co.down_sampling_voxel2(xyz, rgb, 0.0005)
    assert np.array_equal(c, rgb)


# -------------------------------------------------------------------------------------------------------------- (c) Python layer
def test_png_decoding_matches_imread_color(tmp_path):
    from PIL import Image
    ds = importlib.import_module("global-lvba_amd.dataset")
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "rgb.png")
    assert np.array_equal(ds.read_image_bgr(str(tmp_path / "rgb.png")), rgb[:, :, ::-1])
    rgba = np.concatenate([rgb, rng.integers(0, 256, (7, 9, 1), dtype=np.uint8)], 2)
    Image.fromarray(rgba, "RGBA").save(tmp_path / "rgba.png")
    assert np.array_equal(ds.read_image_bgr(str(tmp_path / "rgba.png")), rgb[:, :, ::-1])      # alpha dropped, not blended
    grey = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    Image.fromarray(grey, "L").save(tmp_path / "l.png")
    assert np.array_equal(ds.read_image_bgr(str(tmp_path / "l.png")), np.repeat(grey[:, :, None], 3, 2))
    assert ds.read_image_bgr(str(tmp_path / "rgb.png"), 9, 7).shape == (7, 9, 3)              # camera size: untouched
    assert ds.read_image_bgr(str(tmp_path / "rgb.png"), 18, 14).shape == (14, 18, 3)          # otherwise resized


def test_pcd_xyzrgb_round_trip(tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((500, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    p = str(tmp_path / "c.pcd")
    ds.save_pcd_xyzrgb(p, xyz, rgb)
    raw = open(p, "rb").read()
    hdr = raw[:raw.index(b"DATA binary\n") + 12].decode()
    assert "FIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\n" in hdr and "POINTS 500\n" in hdr
    assert len(raw) - len(hdr) == 16 * 500
    packed = np.frombuffer(raw[len(hdr):], np.uint32).reshape(500, 4)[:, 3]
    assert np.array_equal(packed, 0xFF000000 | (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2])
    x2, c2 = ds.load_pcd_xyzrgb(p)
    assert np.array_equal(x2, xyz) and np.array_equal(c2, rgb)
    ds.save_pcd_xyzrgb(p, np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(ds.load_pcd_xyzrgb(p)[0]) == 0


def test_run_dataset_default_writes_white_landmarks(tmp_path, monkeypatch):
    """Without colorize, run_dataset's outputs are what they were: points3D.txt holds the valid landmarks in white and no PCD
    is written; the pipeline is not handed any images."""
    pipe = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    seen = {}

    def fake_pipeline(*a, **kw):
        seen.update(kw)
        return dict(poses=np.tile(np.r_[np.eye(3).reshape(-1), 0, 0, 0], (2, 1)),
                    visual=dict(Rcw=np.tile(np.eye(3), (2, 1, 1)), tcw=np.zeros((2, 3)), landmarks=np.array([[1.0, 2, 3], [4, 5, 6]]),
                                landmark_valid=np.array([1, 0], np.uint8)))
    monkeypatch.setattr(ds, "load_dataset", lambda p: dict(clouds=[np.zeros((1, 4), np.float32)] * 2, poses=np.zeros((2, 12)),
                                                             timestamps=np.array([1.0, 1.1])))
    monkeypatch.setattr(ds, "load_poses_tum", lambda p, s=1: (np.array([1.0, 1.1]), np.zeros((2, 12))))
    monkeypatch.setattr(ds, "load_colmap_db", lambda p, names, pairs: ([np.zeros((0, 2))] * 2, [np.zeros((0, 2), np.int64)]))
    monkeypatch.setattr(pipe, "run_full_pipeline", fake_pipeline)
    os.makedirs(tmp_path / "data" / "all_image")
    for t in ("1.000000", "1.100000"):
        open(tmp_path / "data" / "all_image" / f"{t}.png", "wb").close()
    out_dir = tmp_path / "out"
    pipe.run_dataset(str(tmp_path / "data"), "db", np.zeros(8), 4, 4, np.eye(3), np.zeros(3), out_dir=str(out_dir))
    assert seen.get("images") is None
    assert open(out_dir / "points3D.txt").read() == "0 1.000000 2.000000 3.000000 255 255 255 0\n"
    assert not any(f.endswith(".pcd") for f in os.listdir(out_dir))
