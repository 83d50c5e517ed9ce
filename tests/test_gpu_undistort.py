"""GPU tests of the undistorted-image export (include/lvba_hip.h "the undistorted images of the COLMAP export"):
every case against the numpy oracle -- the position bit for bit including the NaNs, the mask, n_valid, the images byte for byte,
plain and with gains --, the same bytes for every batching, three closed forms, the coherence claim against the colour fusion, the
refusals, and pipeline.run_dataset's files.  Every comparison is exact."""
import ctypes
import importlib
import json

import numpy as np
import pytest

import undistort_cases as uc
import undistort_oracle as uo

pytestmark = pytest.mark.gpu


def _mods():
    pkg = importlib.import_module("global-lvba_amd")
    return pkg, importlib.import_module("global-lvba_amd.undistort"), importlib.import_module("global-lvba_amd.pipeline")


same_bytes = uc.same_bytes


def same_doubles(a, b):
    """bit for bit, the NaNs in the same places"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same_bytes(np.nan_to_num(a), np.nan_to_num(b))


def cases():
    UN = _mods()[1]
    return uc.basic_cases() + uc.tile_cases(*UN.tile())


_EXPECTED = {}


def expected(c):
    """the oracle's (uv, mask, images, images under gains) of a case, computed once"""
    if c["name"] not in _EXPECTED:
        img, g = uc.images_of(c), uc.gains_of(c)
        uv, mask = uo.position(c["intr"], c["width"], c["height"], **c["opts"])
        _EXPECTED[c["name"]] = (uv, mask, uo.images(img, c["intr"], None, **c["opts"]), uo.images(img, c["intr"], g, **c["opts"]))
    return _EXPECTED[c["name"]]


def run_gpu(c, images, gains=None, **more):
    UN = _mods()[1]
    with UN.Undistorter(c["intr"], c["width"], c["height"], **dict(c["opts"], **more)) as und:
        return und.mask(), und.images(images, gains=gains)


def test_every_case_equals_the_oracle():
    UN = _mods()[1]
    for c in cases():
        uc.check_conditions(c)
        img, g = uc.images_of(c), uc.gains_of(c)
        uv, mask, plain, gained = expected(c)
        pin, size, _ = uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])
        with UN.Undistorter(c["intr"], c["width"], c["height"], **c["opts"]) as und:
            assert und.size == size and und.pinhole == pin and und.n_valid == int((mask != 0).sum()), c["name"]
            assert same_doubles(und.map(), uv), c["name"]
            assert same_bytes(und.mask(), mask), c["name"]
            assert same_bytes(und.images(img), plain), c["name"]
            assert same_bytes(und.images(img, gains=g), gained), c["name"]
            assert same_bytes(und.images(img, gains=np.tile(np.array([65536, 0], np.int64), (c["m"], 3, 1))), plain), c["name"]   # identity


def test_same_bytes_for_any_batching():
    UN = _mods()[1]
    for c in (x for x in cases() if x["m"] >= 3):
        img, g = uc.images_of(c), uc.gains_of(c)
        _, _, plain, gained = expected(c)
        for batch in (1, 2, 0):
            with UN.Undistorter(c["intr"], c["width"], c["height"], max_batch_images=batch, **c["opts"]) as und:
                assert same_bytes(und.images(img), plain) and same_bytes(und.images(img, gains=g), gained), (c["name"], batch)
                parts = np.concatenate([und.images(img[:1], gains=g[:1]), und.images(img[1:], gains=g[1:])])       # several calls
                assert same_bytes(parts, gained), (c["name"], batch)
                assert und.images(img[:0]).shape == (0,) + plain.shape[1:]
        got = [b for _, b in UN.undistort_images(lambda k: img[k], c["intr"], c["width"], c["height"], gains=g, chunk=2, n=c["m"], **c["opts"])]
        assert same_bytes(np.stack(got), gained), c["name"]


def test_closed_forms():
    uc.closed_identity(run_gpu)
    uc.closed_half_pixel(run_gpu)
    uc.closed_constant(run_gpu)


def test_what_the_fusion_reads_from_the_raw_image_is_the_exported_pixel():
    """The coherence claim, on the dyadic case with its distortion: the float32 point ((i - cx') / fx', (j - cy') / fy', 1) of every
    valid target pixel, fused from the single raw image at the identity pose, has the undistorted image's colour, byte for byte,
    with the same gains on both sides -- and the fusion sees exactly the valid pixels."""
    PH = importlib.import_module("global-lvba_amd.photo")
    c = next(x for x in cases() if x["name"] == "dyadic")
    uc.check_conditions(c)
    (fx, fy, cx, cy), (wo, ho), _ = uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])
    i, j = np.meshgrid(np.arange(wo, dtype=np.float64), np.arange(ho, dtype=np.float64))
    pts64 = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i)], -1).reshape(-1, 3)
    pts = pts64.astype(np.float32)
    assert (pts.astype(np.float64) == pts64).all()       # exact in float32: both sides start from the same doubles
    img, g = uc.images_of(c), uc.gains_of(c)
    for gains in (None, g):
        mask, out = run_gpu(c, img, gains)
        assert 0 < int((mask == 0).sum()) < mask.size
        for q in range(c["m"]):
            with PH.PhotoMap(pts, 1, c["intr"], c["width"], c["height"]) as pm:
                pm.add_images(0, np.eye(3)[None], np.zeros((1, 3)), img[q:q + 1], **({} if gains is None else dict(gains=gains[q:q + 1])))
                fused = pm.finish()
            valid = mask.reshape(-1) != 0
            assert np.array_equal(fused["n_views"] == 1, valid) and not fused["n_views"][~valid].any()
            assert same_bytes(fused["rgb"][valid], np.ascontiguousarray(out[q].reshape(-1, 3)[valid][:, ::-1])), (q, gains is None)


def test_invalid_arguments_are_refused():
    pkg, UN, _ = _mods()
    L = pkg._lib
    lib = ctypes.CDLL(L.LIB_PATH)                           # raw prototypes: NULL pointers go through as they are
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.lvba_undistort_create.argtypes = [i32, i32, i32, vp, vp, ctypes.POINTER(vp)]
    lib.lvba_undistort_info.argtypes = [vp, vp, vp, vp, vp]
    lib.lvba_undistort_images.argtypes = [vp, i32, vp, vp, vp]
    lib.lvba_undistort_map.argtypes = [vp, vp, vp]
    lib.lvba_undistort_profile.argtypes = [vp, vp]
    lib.lvba_undistort_tile.argtypes = [vp, vp, vp]
    lib.lvba_undistort_free.argtypes = [vp]
    lib.lvba_undistort_free.restype = None
    lib.lvba_last_error.restype = ctypes.c_char_p
    c = uc.basic_cases()[1]
    W, H, intr = c["width"], c["height"], np.ascontiguousarray(c["intr"])
    ptr = lambda a: a.ctypes.data
    SENTINEL = 0x5A5A
    h = vp(SENTINEL)

    def create(w=W, hh=H, I=intr, out=True, **o):
        h.value = SENTINEL
        opts = UN.undistort_opts() if o else None
        for k, v in o.items():
            setattr(opts, k, v)                                                  # past make_opts' coercion: NaN, negatives
        return lib.lvba_undistort_create(0, w, hh, ptr(I) if I is not None else None, ctypes.byref(opts) if opts is not None else None,
                                         ctypes.byref(h) if out else None)

    def refused(rc):
        return rc == L.ERR_ARG and h.value == SENTINEL                           # nothing written

    assert refused(create(I=None)) and create(out=False) == L.ERR_ARG
    assert refused(create(w=1)) and refused(create(hh=1)) and refused(create(w=-3))
    assert refused(create(out_width=1)) and refused(create(out_height=1)) and refused(create(out_width=-2))
    for k in range(8):
        bad = intr.copy(); bad[k] = np.nan
        assert refused(create(I=bad)), k
    for k in (0, 1):
        bad = intr.copy(); bad[k] = 0.0
        assert refused(create(I=bad)) and b"focal" in lib.lvba_last_error()
    pin = dict(fx=20.0, fy=21.0, cx=18.0, cy=14.0)
    for name in pin:
        for v in (np.nan, np.inf):
            assert refused(create(**dict(pin, **{name: v}))), (name, v)
    assert refused(create(**dict(pin, fy=0.0))) and b"pinhole" in lib.lvba_last_error()
    assert refused(create(**dict(pin, fx=-20.0)))
    assert refused(create(border=-1)) and refused(create(border=256)) and refused(create(max_batch_images=-1))
    assert create(**c["opts"]) == L.OK and h.value not in (None, SENTINEL)
    img, g = uc.images_of(c), uc.gains_of(c)
    _, mask, plain, _ = expected(c)
    out = np.full(plain.shape, 123, np.uint8)
    run = lambda n=c["m"], I=img, G=None, O=out, hh=h: lib.lvba_undistort_images(hh, n, ptr(I) if I is not None else None,
                                                                                  ptr(G) if G is not None else None, ptr(O) if O is not None else None)
    assert run(hh=None) == L.ERR_ARG and run(n=-1) == L.ERR_ARG and run(I=None) == L.ERR_ARG and run(O=None) == L.ERR_ARG
    for (q, k, e), v in {(0, 0, 0): (1 << 14) - 1, (1, 2, 0): (1 << 18) + 1, (1, 1, 1): 65536 * 65280 + 1, (0, 2, 1): -65536 * 65280 - 1}.items():
        bad = g.copy(); bad[q, k, e] = v
        assert run(G=bad) == L.ERR_ARG and b"gains" in lib.lvba_last_error(), (q, k, e)
    assert (out == 123).all()                                                    # the refusals wrote nothing
    ms = np.full(3, -1.0)
    assert lib.lvba_undistort_profile(h, ptr(ms)) == L.OK and (ms == 0.0).all()
    assert lib.lvba_undistort_profile(None, ptr(ms)) == L.ERR_ARG and lib.lvba_undistort_profile(h, None) == L.ERR_ARG
    assert lib.lvba_undistort_info(None, None, None, None, None) == L.ERR_ARG and lib.lvba_undistort_map(None, None, None) == L.ERR_ARG
    t = np.zeros(3, np.int32)
    assert lib.lvba_undistort_tile(None, ptr(t[1:]), ptr(t[2:])) == L.ERR_ARG and not t.any()
    assert run(n=0, I=None, O=None) == L.OK and (out == 123).all()
    assert run() == L.OK and same_bytes(out, plain)                              # still usable
    nv, m2 = ctypes.c_int64(-1), np.zeros(mask.shape, np.uint8)
    assert lib.lvba_undistort_info(h, None, None, None, ctypes.byref(nv)) == L.OK and nv.value == int((mask != 0).sum())   # each may be NULL
    assert lib.lvba_undistort_map(h, None, None) == L.OK and lib.lvba_undistort_map(h, None, ptr(m2)) == L.OK and same_bytes(m2, mask)
    assert lib.lvba_undistort_profile(h, ptr(ms)) == L.OK and (ms >= 0.0).all()
    lib.lvba_undistort_free(h)
    lib.lvba_undistort_free(None)
    assert L.load().lvba_version() == 112
    with pytest.raises(TypeError):
        UN.Undistorter(intr, W, H, no_such_option=1)
    with UN.Undistorter(intr, W, H) as und:
        with pytest.raises(ValueError):
            und.images(img[:, :-1])
        with pytest.raises(ValueError):
            und.images(img, gains=g[:1])
        und.images(img)
        p = und.profile()
        assert sorted(p) == ["download", "kernel", "upload"] and all(v >= 0.0 for v in p.values())


# ------------------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """the small sequence of tests/test_gpu_photo.py's dataset test, written once: (root, tp, images, cfg)"""
    import sqlite3
    from PIL import Image
    ds = importlib.import_module("global-lvba_amd.dataset")
    import test_gpu_colorize as tc
    tp, d, images, cfg = tc._pipeline_data()
    root = tmp_path_factory.mktemp("undistort_seq") / "seq"
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
    return root, tp, images, cfg


def image_rows(path):
    """the image names of images.txt, row by row"""
    return [ln.split()[-1] for ln in open(path).read().splitlines()[::2]]


def test_run_dataset_writes_png_images(sequence, tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    pipe = _mods()[2]
    root, tp, images, cfg = sequence
    out_dir = tmp_path / "out"
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir),
                           undistorted_images=dict(format="png", border=40, max_batch_images=3), **cfg)
    names = image_rows(out_dir / "images.txt")
    assert names == [f"{k}.png" for k in range(len(images))]                    # one row per image, named as the files are
    assert sorted(p.name for p in (out_dir / "images").iterdir()) == sorted(names)
    want = uo.images(images, tp.INTR, None, border=40)
    uv, mask = uo.position(tp.INTR, tp.W, tp.H)
    assert 0 < int((mask == 0).sum()) < mask.size // 2
    for k, name in enumerate(names):
        assert same_bytes(ds.read_image_bgr(str(out_dir / "images" / name)), want[k]), name
    assert same_bytes(ds.read_image_bgr(str(out_dir / "images_mask.png"))[:, :, 0], mask)
    fx, fy, cx, cy = (float(v) for v in tp.INTR[:4])
    assert open(out_dir / "cameras.txt").read() == f"1 PINHOLE {tp.W} {tp.H} {fx!r} {fy!r} {cx!r} {cy!r}\n"
    rep = json.load(open(out_dir / "undistorted.json"))
    assert rep == json.loads(json.dumps(got["undistorted"]))
    assert sorted(rep) == sorted(["size", "pinhole", "n_valid", "profile", "n_files", "format", "options"])
    assert rep["size"] == [tp.W, tp.H] and rep["pinhole"] == [fx, fy, cx, cy] and rep["n_valid"] == int((mask != 0).sum())
    assert rep["n_files"] == len(images) and rep["format"] == "png" and rep["options"]["border"] == 40
    assert sorted(rep["profile"]) == ["download", "kernel", "upload"] and all(v >= 0.0 for v in rep["profile"].values())


def test_run_dataset_writes_jpg_images(sequence, tmp_path):
    from PIL import Image
    pipe = _mods()[2]
    root, tp, images, cfg = sequence
    out_dir = tmp_path / "out"
    pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir),
                     undistorted_images=dict(out_width=241, out_height=181, fx=150.0, fy=149.0, cx=120.5, cy=90.25), **cfg)
    names = image_rows(out_dir / "images.txt")
    assert names == [f"{k}.jpg" for k in range(len(images))]                    # the reference's names
    for name in names:
        with Image.open(out_dir / "images" / name) as im:
            assert im.format == "JPEG" and im.size == (241, 181)
            im.load()
    assert open(out_dir / "cameras.txt").read() == "1 PINHOLE 241 181 150.0 149.0 120.5 90.25\n"


def test_run_dataset_applies_the_exposure_gains(sequence, tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    pipe = _mods()[2]
    root, tp, images, cfg = sequence
    out_dir = tmp_path / "out"
    got = pipe.run_dataset(str(root), "colmap.db", tp.INTR, tp.W, tp.H, tp.RCB, tp.TCI, out_dir=str(out_dir), photo_consistency=True,
                           exposure=dict(rounds=1, min_samples=50), undistorted_images=dict(format="png", apply_exposure=True), **cfg)
    gains = got["exposure"]["gains"]
    assert gains.shape == (len(images), 3, 2)
    print("gains other than the identity:", int((gains != np.array([65536, 0])).any(axis=(1, 2)).sum()), "of", len(gains))
    want = uo.images(images, tp.INTR, gains)
    for k in range(len(images)):
        assert same_bytes(ds.read_image_bgr(str(out_dir / "images" / f"{k}.png")), want[k]), k
    assert (out_dir / "exposure.json").exists() and (out_dir / "undistorted.json").exists()
