"""CPU tests of the SIFT extractor's rule and fixtures (include/lvba_hip.h "SIFT key points and descriptors"): the
library's blur taps against numpy's, the oracle on a blob and under a quarter turn, csrc/sift_device.h on the host against the oracle,
the fragility condition of the fixtures with the orientation tolerance the GPU tests import, the end-to-end floor, and run_dataset's
argument checks."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import match_oracle as mo
import sift_cases as sc
import sift_oracle as so
from host_build import build_check

# The fragile share a fixture may have (the condition of the issue), and what this file measures for the GPU tests:
MAX_FRAGILE_SHARE = 0.02
# 10 x the largest difference of a float orientation between the plain and the perturbed evaluation of the oracle over the
# non-fragile key points of FEATURE_CASES.  Measured: 0.0 (no float orientation moves under a relative 1e-12) -> ORI_TOL 0.0;
# test_fragile_share_and_orientation_tolerance re-measures it.
ORI_TOL = 10 * 0.0
# 0.9 x the share of the oracle's matches of the warp pair that lie within 2 px of the similarity.  Measured: 68 of 71 = 0.9577.
WARP_MATCH_FLOOR = 0.9 * 0.9577
WARP_MAX_PX = 2.0


def warp_share(kp_a, kp_b, matches):
    err = np.linalg.norm(sc.similarity(kp_a[matches[:, 0], :2]) - kp_b[matches[:, 1], :2].astype(np.float64), axis=1)
    return float((err <= WARP_MAX_PX).mean()), len(matches)


@pytest.fixture(scope="module")
def ft():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("global-lvba_amd.features")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/sift_device.h compiled for the host, without contraction, walked as the kernels walk it (tests/sift_check.cpp)"""
    lib = ctypes.CDLL(build_check("sift_check", tmp_path_factory.mktemp("emul_sift")))
    V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emul_pow2.restype = D
    lib.emul_pow2.argtypes = [D]
    lib.emul_refine.argtypes = [V, I, I, I, D, D, V, V]
    lib.emul_ori_hist.restype = None
    lib.emul_ori_hist.argtypes = [V, I, I, I, I, D, D, D, D, V]
    lib.emul_ori_peaks.argtypes = [V, I, V]
    lib.emul_desc_bins.restype = None
    lib.emul_desc_bins.argtypes = [V, I, I, I, I, D, D, D, ctypes.c_float, V]
    lib.emul_desc_bytes.restype = None
    lib.emul_desc_bytes.argtypes = [V, V]
    return lib


def test_blur_taps_against_numpy(ft):
    """Within one fp32 ulp per tap of numpy's fp64 Gaussian, sum 1 to 1e-6, radius ceil(4 sigma); host only."""
    for opts in ({}, dict(first_octave=0), dict(n_intervals=4, sigma0=2.0), dict(n_intervals=2, sigma0=1.2, first_octave=0)):
        o = so.options(**opts)
        for level in range(o["n_intervals"] + 3):
            t = ft.blur_taps(level, **opts)
            g, r = so.numpy_taps(o, level)
            assert t.dtype == np.float32 and len(t) == 2 * r + 1 and r == math.ceil(4.0 * so.level_sigma(o, level))
            assert (np.abs(t.astype(np.float64) - g) <= np.spacing(g.astype(np.float32)).astype(np.float64)).all(), (opts, level)
            assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 1e-6
            np.testing.assert_array_equal(t, t[::-1])
    L = importlib.import_module("global-lvba_amd._lib")
    for bad in (dict(level=-1), dict(level=6), dict(level=0, sigma0=1.0), dict(level=0, n_intervals=2, sigma0=3.5)):
        with pytest.raises(L.LvbaError) as e:
            ft.blur_taps(**bad)
        assert e.value.code == L.ERR_ARG


def test_options_struct_matches_the_header():
    """lvba_sift_opts: the defaults are SiftGPU's five parameters (the layout against the header: tests/test_abi.py)."""
    L = importlib.import_module("global-lvba_amd._lib")
    assert ctypes.sizeof(L.SiftOpts) == 56
    o = importlib.import_module("global-lvba_amd.features").sift_opts()
    assert (o.first_octave, o.n_intervals, o.sigma0, o.dog_threshold, o.edge_threshold, o.orientation_window, o.max_orientations,
            o.max_features, o.chunk_images, o.reserved) == (-1, 3, 1.6, 0.01, 12.0, 3.0, 2, 8192, 0, 0)


def test_oracle_finds_a_blob():
    """One Gaussian blob of sigma s at a sub-pixel place: found within 0.1 px, and within 10 % of the scale at which the DoG of the
    rule peaks on it.  At the blob's centre G(k sigma) - G(sigma), k = 2^(1/S), responds with 1 / (s^2 + k^2 sigma^2) -
    1 / (s^2 + sigma^2), whose magnitude is largest at sigma = s / sqrt(k): that, not s, is the sigma the rule assigns."""
    o, taps = so.options(), sc.library_taps()
    for s, cx, cy in ((3.0, 30.3, 25.7), (2.0, 20.6, 22.2), (4.5, 31.4, 30.8)):
        yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
        img = np.clip(np.rint(100 + 120 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))), 0, 255).astype(np.uint8)
        c = so.candidates(so.pyramid(img, o, taps), o)
        assert len(c) == 1
        x, y, sigma = (float(v) for v in c[0]["xys"])
        assert math.hypot(x - cx, y - cy) <= 0.1
        assert abs(sigma - s / math.sqrt(2.0 ** (1.0 / 3.0))) <= 0.1 * s / math.sqrt(2.0 ** (1.0 / 3.0))


def test_oracle_descriptor_under_a_quarter_turn():
    """np.rot90 of a level moves the pixel (x, y) to (y, w - 1 - x) and turns every gradient by -90 degrees.  With the orientation
    held, the frame turns by +90 degrees against the content: the cell (r, c) goes to (3 - c, r) and the direction o to o - 2.
    The same bytes up to that permutation, for every key point of the fixture."""
    img, opts, ref = sc.reference("bgr_96x80")
    m = so.Libm()
    perm = np.zeros(128, np.int64)
    for r in range(4):
        for c in range(4):
            for k in range(8):
                perm[(4 * (3 - c) + r) * 8 + (k - 2) % 8] = (4 * r + c) * 8 + k
    n = 0
    for cand, feats in zip(ref["candidates"], ref["features"]):
        L = ref["pyramid"][cand["k"]][0][cand["l"]]
        w = L.shape[1]
        turned = dict(cand, x=cand["y"], y=w - 1 - cand["x"], ox=cand["oy"], oy=-cand["ox"])
        L2 = np.ascontiguousarray(np.rot90(L))
        for theta, b in feats:
            b2 = so.descriptor_bytes(so.descriptor_bins(L2, turned, theta, m), m)
            np.testing.assert_array_equal(b2, b[perm])
            n += 1
    assert n >= 40


def test_device_header_on_the_host_equals_the_oracle(emul):
    """The kernels' scalar pieces without the GPU: the refinement bit for bit, 2^z bit for bit, the peak picking and the
    quantisation bit for bit on the oracle's sums; the histogram and the descriptor sums, which go through two libms, to 1e-12."""
    for z in (-1.0, -0.3, 0.0, 0.5, 1.0 / 3.0, 1.17, 2.0, 3.999):
        assert emul.emul_pow2(z) == so.pow2(z) and abs(so.pow2(z) / 2.0 ** z - 1.0) < 1e-15
    n_ref = n_feat = 0
    for name, _, _ in sc.FEATURE_CASES:
        img, opts, ref = sc.reference(name)
        o = so.options(**opts)
        S = o["n_intervals"]
        for G, D in ref["pyramid"]:
            Dc = np.ascontiguousarray(D)
            h, w = D.shape[1:]
            for l, y, x in so.extrema(D, o):
                pos, off = np.array([x, y, l], np.int32), np.zeros(3)
                ok = emul.emul_refine(Dc.ctypes.data, w, h, S, o["dog_threshold"], o["edge_threshold"], pos.ctypes.data, off.ctypes.data)
                want = so.refine(D, o, int(x), int(y), int(l))
                assert bool(ok) == (want is not None)
                if want is not None:
                    assert tuple(pos) == want[:3] and tuple(off) == want[3:]
                n_ref += 1
        m = so.Libm()
        for cand, feats in zip(ref["candidates"], ref["features"]):
            L = np.ascontiguousarray(ref["pyramid"][cand["k"]][0][cand["l"]])
            h, w = L.shape
            hist = np.zeros(36)
            emul.emul_ori_hist(L.ctypes.data, w, h, cand["x"], cand["y"], cand["ox"], cand["oy"], cand["sig"], o["orientation_window"],
                               hist.ctypes.data)
            want = so.orientation_histogram(L, cand, o, m)
            np.testing.assert_allclose(hist, want, rtol=1e-12, atol=0)
            theta = np.zeros(4)
            k = emul.emul_ori_peaks(want.ctypes.data, o["max_orientations"], theta.ctypes.data)
            assert list(theta[:k]) == so.orientation_peaks(want, o["max_orientations"])
            for t, b in feats:
                acc = np.zeros(128)
                emul.emul_desc_bins(L.ctypes.data, w, h, cand["x"], cand["y"], cand["ox"], cand["oy"], cand["sig"], float(t), acc.ctypes.data)
                want_acc = so.descriptor_bins(L, cand, t, m)
                np.testing.assert_allclose(acc, want_acc, rtol=1e-12, atol=1e-300)
                out = np.zeros(128, np.uint8)
                emul.emul_desc_bytes(want_acc.ctypes.data, out.ctypes.data)
                np.testing.assert_array_equal(out, b)
                n_feat += 1
    assert n_ref > 100 and n_feat > 80


def test_oracle_order_cap_and_edge_images():
    """The canonical order; the max_features rule; a constant image and an image whose only extremum lies on the border."""
    img, opts, ref = sc.reference("bgr_96x80")
    key = [(c["k"],) for c in ref["candidates"]]
    assert key == sorted(key) and len({c["octave"] for c in ref["candidates"]}) >= 3
    assert max(len(f) for f in ref["features"]) == 2 and ref["count"] == len(ref["keypoints"])
    o = so.options(max_features=20)
    kp, ds, count, src = so.assemble(ref["candidates"], ref["features"], o)
    assert count == ref["count"] > 20 and len(kp) == 20 and (np.diff(src) >= 0).all()
    full = ref["keypoints"]
    assert kp[:, 2].min() >= np.sort(full[:, 2])[-20] and set(map(tuple, kp)) <= set(map(tuple, full))
    taps = sc.library_taps()
    assert so.extract(sc.constant(20, 16), so.options(), taps)[2] == 0
    o0, t0 = so.options(first_octave=0), sc.library_taps(first_octave=0)
    pyr = so.pyramid(sc.border_extremum(), o0, t0)
    assert float(np.abs(pyr[0][1][1:4, :, 0]).max()) > 10 * (0.5 * o0["dog_threshold"]) / 3       # it is there, in column 0
    assert all(len(so.extrema(D, o0)) == 0 for _, D in pyr)


def test_fragile_share_and_orientation_tolerance():
    """At most 2 % of the key points of each fixture change their number of orientations or a descriptor byte when every atan2,
    exp, sqrt, cos and sin result moves by a relative 1e-12 -- a thousand times a libm's error; ORI_TOL is 10 x the largest
    orientation difference over the rest, the factor being the room for the device's summation."""
    worst = 0.0
    for name, _, _ in sc.FEATURE_CASES:
        ref = sc.reference(name)[2]
        assert len(ref["candidates"]) >= 15
        share = float(ref["fragile"].mean())
        print(f"{name}: {len(ref['candidates'])} key points, {ref['count']} features, fragile share {share:.4f}, "
              f"largest orientation difference {ref['dtheta']:.3e}")
        assert share <= MAX_FRAGILE_SHARE
        worst = max(worst, ref["dtheta"])
    assert ORI_TOL == 10 * worst


def test_warp_pair_floor():
    """The oracle's features of a texture and of its warp by a similarity (30 degrees, 1.4, a shift) through the matcher's
    oracle: WARP_MATCH_FLOOR is 0.9 x the share of the matches within 2 px of the similarity."""
    imgs, feats = sc.warp_reference()
    m, _ = mo.match_pair([feats[0][1], feats[1][1]], 0, 1)
    share, n = warp_share(feats[0][0], feats[1][0], m)
    print(f"warp pair: {[len(k) for k, _ in feats]} features, {n} matches, share within {WARP_MAX_PX} px {share:.4f}")
    assert n >= 50 and abs(WARP_MATCH_FLOOR - 0.9 * share) < 1e-4


def test_run_dataset_feature_arguments(tmp_path, monkeypatch):
    """features="images" refuses matching="db" before it reads anything and never
    opens the database."""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    args = (str(tmp_path), "db.db", np.ones(8), 64, 48, np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="matching"):
        pl.run_dataset(*args, features="images")
    with pytest.raises(ValueError, match="matching"):
        pl.run_dataset(*args, features="images", matching="db")
    with pytest.raises(ValueError, match="features"):
        pl.run_dataset(*args, features="sift")
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    for t in (0.5, 1.5):
        ds.save_pcd(str(tmp_path / "all_pcd_body" / f"{t}.pcd"), rng.normal(size=(10, 4)).astype(np.float32))
        (tmp_path / "all_image" / f"{t}.png").write_bytes(b"")
    (tmp_path / "all_pcd_body" / "lidar_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    (tmp_path / "all_image" / "image_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    calls = []
    monkeypatch.setattr(pl, "run_full_pipeline", lambda *a, **k: calls.append((a, k)) or {})
    monkeypatch.setattr(ds, "load_colmap_db", lambda *a, **k: pytest.fail("features='images' opens no database"))
    monkeypatch.setattr(ds, "load_colmap_descriptors", lambda *a, **k: pytest.fail("features='images' opens no database"))
    seen = []

    def fake_extract(read_image, n_images, **kw):
        seen.append((n_images, kw))
        return [np.zeros((3, 4), np.float32)] * n_images, [np.zeros((3, 128), np.uint8)] * n_images
    monkeypatch.setattr(pl, "extract_image_features", fake_extract)
    pl.run_dataset(*args, features="images", matching="guided", feature_opts=dict(max_features=100))
    assert seen == [(2, dict(device=0, max_features=100))]
    (a, k), = calls
    assert "match_fn" in k and [x.shape for x in a[-3]] == [(3, 2), (3, 2)]
