"""GPU tests of the multi-view colour fusion (lvba_photo_*, csrc/photo.hip) against the numpy restatement
(tests/photo_oracle.py) on the room of tests/photo_cases.py.  Sums, n_views, rgb and sigma compare exactly -- sigma as bytes, NaNs
included: the fixture's margin condition (photo_cases.check_margins, asserted on the CPU) is what allows that."""
import ctypes
import importlib
import json
import math

import numpy as np
import pytest

import covis_cases as cc
import photo_cases as pc
import photo_oracle as po

pytestmark = pytest.mark.gpu


def _mods():
    return (importlib.import_module("global-lvba_amd"), importlib.import_module("global-lvba_amd.photo"),
            importlib.import_module("global-lvba_amd.visual"), importlib.import_module("global-lvba_amd.pipeline"))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_gpu(points, images, depth, intr, Rcw, tcw, calls=None, finish_between=False, n_images=None, **opts):
    """dict(sums=(n_views, s1, s2), n_views, rgb, sigma, summary): images added by calls [(first, count), ...] (default: one call)"""
    _, PH, V, _ = _mods()
    M = len(images) if n_images is None else n_images
    W, H = images.shape[2], images.shape[1]
    dset = V.DepthImages.upload(depth) if depth is not None else None
    try:
        with PH.PhotoMap(points, M, intr, W, H, depth=dset, **opts) as pm:
            for a, m in (calls if calls is not None else [(0, M)]):
                pm.add_images(a, Rcw[a:a + m], tcw[a:a + m], images[a:a + m])
                if finish_between:
                    pm.finish()
            out = pm.finish()
            out["sums"] = pm.sums()
            return out
    finally:
        if dset is not None:
            dset.close()


def assert_equals_oracle(got, e, take=slice(None), msg=""):
    nv, s1, s2 = got["sums"]
    assert same_bytes(nv, e["n_views"][take]) and same_bytes(s1, e["s1"][take]) and same_bytes(s2, e["s2"][take]), msg
    assert same_bytes(got["n_views"], e["n_views"][take]) and same_bytes(got["rgb"], np.ascontiguousarray(e["rgb"][take])), msg
    assert same_bytes(got["sigma"], np.ascontiguousarray(e["sigma"][take])), msg


def scene_args(s, with_depth=True, M=cc.N_IMAGES, n=None):
    return (s["points"][:n], s["images"][:M], s["depth"][:M] if with_depth else None, s["intr"], s["Rcw"][:M], s["tcw"][:M])


# ------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
@pytest.mark.parametrize("option_set", range(len(pc.OPTION_SETS)))
def test_every_point_equals_the_oracle(size, option_set):
    with_depth, opts = pc.split(pc.OPTION_SETS[option_set])
    e = pc.expected(size, **pc.OPTION_SETS[option_set])
    got = run_gpu(*scene_args(pc.scene(size), with_depth), **opts)
    assert (e["n_views"] >= 3).any() and (e["n_views"] == 0).any()
    assert_equals_oracle(got, e, msg=str(pc.OPTION_SETS[option_set]))


# ------------------------------------------------------------------------------------------------------------ 2. chunk edges
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_chunk_edges(size):
    """the first 0, 1, 63, 64, 255, 256, 257 and all points (a workgroup owns 256), and the first 21, 2 and 1 images"""
    s = pc.scene(size)
    e = pc.expected(size)
    for n in pc.POINT_COUNTS:
        got = run_gpu(*scene_args(s, n=n))
        assert len(got["n_views"]) == n
        assert_equals_oracle(got, e, slice(0, n), f"{n} points")
        assert got["summary"]["n_points"] == n
    for M in pc.M_VALUES[1:]:
        args = scene_args(s, M=M)
        assert_equals_oracle(run_gpu(*args), po.evaluate(*args), msg=f"{M} images")


# ---------------------------------------------------------------------------------------------------- 3. batching independence
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_same_bytes_for_any_batching(size):
    s = pc.scene(size)
    args = scene_args(s)
    M = cc.N_IMAGES
    ref = run_gpu(*args)
    assert_equals_oracle(ref, pc.expected(size))
    one = [(k, 1) for k in range(M)]
    for kw in (dict(calls=one), dict(calls=one[::-1]), dict(max_batch_images=1), dict(max_batch_images=2),
               dict(calls=[(5, 16), (0, 5)], max_batch_images=3), dict(calls=[(0, 2), (2, 3), (5, 16)], finish_between=True)):
        got = run_gpu(*args, **kw)
        for a, b in zip(got["sums"], ref["sums"]):
            assert same_bytes(a, b), kw
        assert same_bytes(got["rgb"], ref["rgb"]) and same_bytes(got["sigma"], ref["sigma"]) and same_bytes(got["n_views"], ref["n_views"]), kw
        assert _plain(got["summary"]) == _plain(ref["summary"]), kw
        assert np.float64(got["summary"]["mean_sigma"]).tobytes() == np.float64(ref["summary"]["mean_sigma"]).tobytes(), kw


# ----------------------------------------------------------------------------------------------------------- 4. pixel edges
def test_pixel_edges_in_exact_arithmetic():
    """R = I, t = 0, no distortion, fx = fy = 64, cx = cy = 32 and dyadic points: u = 64 x + 32 is exact on the host and on the
    device alike (a product by a power of two, a sum of dyadic numbers, and Z = 1), so these points sit ON the boundaries and are
    exempt from the margin condition, whose only purpose is to keep an ulp of the projection's division away from a decision."""
    c = pc.pixel_edge_case()
    R, t = np.eye(3)[None], np.zeros((1, 3))
    got = run_gpu(c["points"], c["image"], None, c["intr"], R, t)
    e = po.evaluate(c["points"], c["image"], None, c["intr"], R, t)
    nv, s1, s2 = got["sums"]
    assert same_bytes(nv, e["n_views"]) and same_bytes(s1, e["s1"]) and same_bytes(s2, e["s2"])
    u, v, W, H = c["u"], c["v"], c["W"], c["H"]
    img = c["image"][0].astype(np.int64)

    def at(uu, vv):
        k = np.flatnonzero((u == uu) & (v == vv))
        assert len(k) >= 1
        return int(nv[k[0]]), s1[k[0]].astype(np.int64)

    n, c16 = at(0.0, 0.0)                                                        # u = 0, v = 0 is sampled: texel (0, 0) alone
    assert n == 1 and (c16 == 256 * img[0, 0]).all()
    for vv in (0.0, 17 + 1 / 256):
        assert at(float(W - 1), vv)[0] == 0                                      # u = w - 1 is not
    assert at(5 + 255 / 256, float(H - 1))[0] == 0 and at(40.0, float(H - 1))[0] == 0          # nor v = h - 1
    assert at(-1 / 256, 0.0)[0] == 0 and at(64.5, 0.0)[0] == 0
    n, c16 = at(W - 1 - 1 / 256, 0.0)                                            # u = w - 1 - 2^-8 reads column w - 1 with weight 255
    assert n == 1 and (c16 == ((256 * (1 * img[0, W - 2] + 255 * img[0, W - 1]) + 128) >> 8)).all()
    n, c16 = at(40.0, H - 1 - 1 / 256)                                           # v likewise: row h - 1 with weight 255
    assert n == 1 and (c16 == ((256 * (1 * img[H - 2, 40] + 255 * img[H - 1, 40]) + 128) >> 8)).all()
    n, c16 = at(1 / 256, 17 + 1 / 256)                                           # fractions 1/256 in both
    want = 255 * 255 * img[17, 0] + 1 * 255 * img[17, 1] + 255 * 1 * img[18, 0] + 1 * 1 * img[18, 1]
    assert n == 1 and (c16 == ((want + 128) >> 8)).all()
    n, c16 = at(255 / 256, 63 + 255 / 256)                                       # fractions 255/256 in both
    want = 1 * 1 * img[63, 0] + 255 * 1 * img[63, 1] + 1 * 255 * img[64, 0] + 255 * 255 * img[64, 1]
    assert n == 1 and (c16 == ((want + 128) >> 8)).all()
    n, c16 = at(1.0, 0.0)                                                        # fraction exactly 0 on the next texel
    assert n == 1 and (c16 == 256 * img[0, 1]).all()
    assert nv[-2] == 0 and nv[-1] == 0                                           # Z = 0, and behind the camera
    inside = (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    np.testing.assert_array_equal(nv, inside.astype(np.int32))


# -------------------------------------------------------------------------------------------------------- 5. the closed form
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_constant_colour_closed_form(size):
    """image k one colour: every sample is exactly 256 colour; sums, rgb and sigma follow from which images see a point"""
    s = pc.scene(size)
    img, colours = pc.constant_images(size)
    got = run_gpu(s["points"], img, s["depth"], s["intr"], s["Rcw"], s["tcw"])
    n, S1, S2, rgb, N = pc.closed_form(pc.expected(size)["seen"], colours)
    nv, s1, s2 = got["sums"]
    assert same_bytes(nv, n) and same_bytes(s1, S1) and same_bytes(s2, S2) and same_bytes(got["rgb"], rgb)
    assert np.isnan(got["sigma"][n < 2]).all()
    for k in np.flatnonzero(n >= 2):
        want = math.sqrt(((float(N[k, 0]) + float(N[k, 1])) + float(N[k, 2])) / (3.0 * 65536.0 * float(int(n[k]) ** 2)))
        assert got["sigma"][k] == want, k


# ------------------------------------------------------------------------------------------------------------ 6. the summary
@pytest.mark.parametrize("size", range(len(cc.SIZES)))
def test_summary(size):
    """integers exact; mean_sigma within (n_valid + 1) 2^-53 relative of math.fsum over the oracle's values / n_valid -- the terms
    are non-negative, so any summation order stays inside that --; two calls give the same bytes"""
    for kw in (dict(), dict(min_views=3), dict(depth=False)):
        with_depth, opts = pc.split(kw)
        e = pc.expected(size, **kw)
        args = scene_args(pc.scene(size), with_depth)
        a, b = run_gpu(*args, **opts)["summary"], run_gpu(*args, **opts)["summary"]
        want = e["summary"]
        for k in ("n_points", "n_seen", "n_valid", "n_samples"):
            assert a[k] == want[k] and type(a[k]) is int, (kw, k)
        assert want["n_valid"] > 100
        print(f"{kw}: mean_sigma {a['mean_sigma']!r}, fsum {want['mean_sigma']!r}")
        assert abs(a["mean_sigma"] - want["mean_sigma"]) <= (want["n_valid"] + 1) * 2.0 ** -53 * want["mean_sigma"], kw
        assert a["mean_views"] == want["mean_views"]
        assert np.float64(a["mean_sigma"]).tobytes() == np.float64(b["mean_sigma"]).tobytes()
        assert len(a["ms"]) == 4 and all(x >= 0 for x in a["ms"]) and a["ms"][1] > 0


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_invalid_arguments_are_refused():
    pkg, PH, V, _ = _mods()
    L = pkg._lib
    lib = ctypes.CDLL(L.LIB_PATH)                           # raw prototypes: NULL pointers go through as they are
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.lvba_photo_create.argtypes = [i32, i64, vp, i32, i32, i32, vp, vp, vp, ctypes.POINTER(vp)]
    lib.lvba_photo_add_images.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.lvba_photo_finish.argtypes = [vp, vp, vp, vp, vp]
    lib.lvba_photo_sums.argtypes = [vp, vp, vp, vp]
    lib.lvba_photo_free.argtypes = [vp]
    lib.lvba_photo_free.restype = None
    lib.lvba_last_error.restype = ctypes.c_char_p
    s = pc.scene(1)
    W, H, M = s["W"], s["H"], cc.N_IMAGES
    ptr = lambda a: a.ctypes.data
    pts, intr = s["points"], np.ascontiguousarray(s["intr"])
    n = len(pts)
    SENTINEL = 0x5A5A
    h = vp(SENTINEL)

    def create(dev=0, n=n, P=pts, M=M, w=W, hh=H, I=intr, depth=None, out=True, **o):
        h.value = SENTINEL
        opts = PH.photo_opts() if o else None
        for k, v in o.items():
            setattr(opts, k, v)                                                  # past make_opts' coercion: NaN, negatives
        return lib.lvba_photo_create(dev, n, ptr(P) if P is not None else None, M, w, hh, ptr(I) if I is not None else None,
                                     depth, ctypes.byref(opts) if opts is not None else None, ctypes.byref(h) if out else None)

    def refused(rc):
        return rc == L.ERR_ARG and h.value == SENTINEL                           # nothing written

    assert refused(create(P=None)) and refused(create(I=None)) and create(out=False) == L.ERR_ARG
    assert refused(create(n=-1)) and refused(create(n=2 ** 32))
    assert refused(create(w=1)) and refused(create(hh=1))
    assert refused(create(M=0)) and refused(create(M=32769))
    for k in range(8):
        bad = intr.copy(); bad[k] = np.nan
        assert refused(create(I=bad)), k
    for k in (0, 1):
        bad = intr.copy(); bad[k] = 0.0
        assert refused(create(I=bad)) and b"focal" in lib.lvba_last_error()
    for name in ("occlusion_rel", "occlusion_abs", "max_depth"):
        for v in (-1e-3, np.nan, np.inf):
            assert refused(create(**{name: v})), (name, v)
    assert refused(create(min_views=1)) and refused(create(min_views=0)) and refused(create(max_batch_images=-1))
    with V.DepthImages.upload(s["depth"][:5]) as few, V.DepthImages.upload(pc.scene(0)["depth"]) as other_size:
        assert refused(create(depth=few._h)) and refused(create(depth=other_size._h))
        assert b"depth set" in lib.lvba_last_error()
    R, t, img = np.ascontiguousarray(s["Rcw"]), np.ascontiguousarray(s["tcw"]), s["images"]
    with V.DepthImages.upload(s["depth"]) as depth:
        assert create(depth=depth._h) == L.OK and h.value not in (None, SENTINEL)
        add = lambda first, m, R=R, t=t, img=img, hh=h: lib.lvba_photo_add_images(
            hh, first, m, ptr(R[first:]) if R is not None else None, ptr(t[first:]) if t is not None else None,
            ptr(img[first:]) if img is not None else None)
        # finish() before any image: nothing is seen
        summ = L.PhotoSummary()
        nv, rgb, sigma = np.full(n, 7, np.int32), np.full((n, 3), 7, np.uint8), np.zeros(n)
        assert lib.lvba_photo_finish(h, ctypes.byref(summ), ptr(nv), ptr(rgb), ptr(sigma)) == L.OK
        assert not nv.any() and not rgb.any() and np.isnan(sigma).all()
        assert (summ.n_points, summ.n_seen, summ.n_valid, summ.n_samples) == (n, 0, 0, 0) and math.isnan(summ.mean_sigma)
        assert add(0, 1, hh=None) == L.ERR_ARG
        assert add(-1, 2) == L.ERR_ARG and add(0, -1) == L.ERR_ARG and add(M, 1) == L.ERR_ARG and add(M - 1, 2) == L.ERR_ARG
        assert add(0, 2, R=None) == L.ERR_ARG and add(0, 2, t=None) == L.ERR_ARG and add(0, 2, img=None) == L.ERR_ARG
        badR = R.copy(); badR[1, 0, 0] = np.nan
        assert add(0, 2, R=badR) == L.ERR_ARG and b"camera 1: non-finite rotation" in lib.lvba_last_error()
        badt = t.copy(); badt[0, 2] = np.inf
        assert add(0, 2, t=badt) == L.ERR_ARG and b"non-finite translation" in lib.lvba_last_error()
        before = np.zeros(n, np.int32)
        assert lib.lvba_photo_sums(h, ptr(before), None, None) == L.OK and not before.any()        # the refusals added nothing
        assert add(3, 4) == L.OK
        assert add(6, 2) == L.ERR_ARG and b"added before" in lib.lvba_last_error()                 # image 6 a second time
        assert add(0, 4) == L.ERR_ARG                                                              # image 3 a second time
        assert add(0, 3) == L.OK and add(7, M - 7) == L.OK                                         # still usable
        filled = bytes(summ)
        assert lib.lvba_photo_finish(None, ctypes.byref(summ), None, None, None) == L.ERR_ARG and bytes(summ) == filled
        assert lib.lvba_photo_finish(h, None, None, None, None) == L.ERR_ARG
        assert lib.lvba_photo_sums(None, None, None, None) == L.ERR_ARG
        assert lib.lvba_photo_finish(h, ctypes.byref(summ), ptr(nv), None, ptr(sigma)) == L.OK     # each per-point output may be NULL
        e = pc.expected(1)
        assert same_bytes(nv, e["n_views"]) and same_bytes(sigma, e["sigma"]) and summ.n_samples == e["summary"]["n_samples"]
        lib.lvba_photo_free(h)
        lib.lvba_photo_free(None)
    assert pkg._lib.load().lvba_version() == 112
    with pytest.raises(TypeError):
        PH.PhotoMap(pts, M, intr, W, H, no_such_option=1)


def test_non_finite_points_keep_their_index():
    s = pc.scene(1)
    e = pc.expected(1)
    pts = s["points"].copy()
    seen = np.flatnonzero(e["n_views"] > 0)                                      # they would have been seen
    bad = {int(seen[0]): (np.nan, 0), int(seen[len(seen) // 2]): (np.inf, 1), int(seen[len(seen) // 2 + 1]): (-np.inf, 2),
           int(seen[-1]): (np.nan, 2)}
    for k, (v, axis) in bad.items():
        pts[k, axis] = v
    got = run_gpu(pts, s["images"], s["depth"], s["intr"], s["Rcw"], s["tcw"])
    keep = np.ones(len(pts), bool)
    keep[list(bad)] = False
    assert not got["n_views"][~keep].any() and not got["rgb"][~keep].any() and np.isnan(got["sigma"][~keep]).all()
    assert same_bytes(got["n_views"][keep], e["n_views"][keep]) and same_bytes(got["sigma"][keep], e["sigma"][keep])
    assert same_bytes(got["sums"][2][keep], e["s2"][keep])


# ------------------------------------------------------------------------------------------------------------ 8. the pipeline
def _plain(summary):
    return {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in summary.items() if k != "ms"}


def test_run_full_pipeline_with_photo_consistency():
    pkg, PH, V, pipe = _mods()
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    args = (d["clouds"], d["odo"], d["times"], d["img_t"], d["odo"], tp.RCB, tp.TCI, tp.INTR, tp.W, tp.H, d["kps"], d["pairs"], d["matches"])
    out = pipe.run_full_pipeline(*args, images=images, photo_consistency=True, **cfg)
    assert sorted(out["photo_consistency"]) == ["after", "before"]
    v = out["visual"]
    sets = dict(after=(out["poses"], v["Rcw"], v["tcw"]), before=(out["poses_before"], v["Rcw_before"], v["tcw_before"]))
    with pkg.Scans([c[:, :3] for c in d["clouds"]]) as scans:
        for name, (x, Rcw, tcw) in sets.items():
            xyz, rgb, n_views, sigma = out["fused_" + name]
            assert xyz is out["colored_" + name][0] and len(xyz) > 1000
            assert rgb.shape == (len(xyz), 3) and n_views.shape == sigma.shape == (len(xyz),)
            summary = out["photo_consistency"][name]
            assert sorted(summary) == sorted(["n_points", "n_seen", "n_valid", "n_samples", "mean_sigma", "mean_views", "ms"])
            assert summary["n_points"] == len(xyz) and summary["n_seen"] > 0
            print(name, summary)
            with V.DepthImages.render(scans, x, d["times"], d["img_t"], Rcw, tcw, tp.INTR, tp.W, tp.H) as depth:
                direct = PH.photo_consistency(xyz, lambda k: images[k], Rcw, tcw, tp.INTR, tp.W, tp.H, depth=depth, chunk=3)
            assert _plain(direct["summary"]) == _plain(summary), name
            assert same_bytes(direct["rgb"], rgb) and same_bytes(direct["sigma"], sigma) and same_bytes(direct["n_views"], n_views)


def test_run_dataset_writes_the_report(tmp_path):
    import sqlite3
    from PIL import Image
    pkg, PH, V, pipe = _mods()
    ds = importlib.import_module("global-lvba_amd.dataset")
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    root = tmp_path / "seq"
    (root / "all_pcd_body").mkdir(parents=True); (root / "all_image").mkdir()
    for t, c in zip(d["times"], d["clouds"]):
        ds.save_pcd(str(root / "all_pcd_body" / f"{t:.6f}.pcd"), np.concatenate([c[:, :3], np.zeros((len(c), 1), np.float32)], 1))
    ds.write_poses_tum(str(root / "all_pcd_body" / "lidar_poses.txt"), d["times"], d["odo"])
    for k, t in enumerate(d["img_t"]):
        Image.fromarray(np.ascontiguousarray(images[k][:, :, ::-1]), "RGB").save(root / "all_image" / f"{t:.6f}.png")
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
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir),
                           photo_consistency=dict(min_views=3), **cfg)
    rep = json.load(open(out_dir / "photo_consistency.json"))
    assert sorted(rep) == ["after", "before", "options"] and rep["options"]["min_views"] == 3
    assert sorted(rep["options"]) == sorted(po.DEFAULTS)
    for name in ("after", "before"):
        assert _plain(rep[name]) == _plain(got["photo_consistency"][name]) and rep[name]["n_seen"] > 0
        assert len(got["fused_" + name][0]) == rep[name]["n_points"]
    assert not (out_dir / "colored_merged_after.pcd").exists()                  # colorize stayed off: only the report is written
