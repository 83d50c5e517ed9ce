"""CPU tests of the undistorted-image export (include/lvba_hip.h "the undistorted images of the COLMAP export"):
the oracle against the rule as plain loops, the device header compiled for the host against the oracle bit for bit, three closed
forms that need no oracle, the conditions each case is there for, the text files of the export, and the argument refusals of
pipeline.run_dataset that need no device.  Every comparison is exact."""
import ctypes
import importlib

import numpy as np
import pytest

import undistort_cases as uc
import undistort_oracle as uo
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/undistort_device.h compiled for the host with g++ -ffp-contract=off -Wall -Werror (tests/undistort_check.cpp)"""
    lib = ctypes.CDLL(build_check("undistort_check", tmp_path_factory.mktemp("emul_undistort")))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.emul_map.argtypes = [P, I, I, P, I, I, P, P]
    lib.emul_images.argtypes = [P, I, I, P, I, I, I, I, P, P, P]
    lib.emul_tile.argtypes = [P]
    lib.emul_map.restype = lib.emul_images.restype = lib.emul_tile.restype = None
    return lib


same_bytes = uc.same_bytes


def host_tile(emul):
    t = np.zeros(4, np.int32)
    emul.emul_tile(t.ctypes.data)
    return tuple(int(v) for v in t)


def host_run(emul, c, images, gains=None):
    """(uv, mask, out) of the compiled header"""
    pin, (wo, ho), border = uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])
    intr, pin = np.ascontiguousarray(c["intr"], np.float64), np.array(pin, np.float64)
    uv, mask = np.zeros((ho, wo, 2)), np.zeros((ho, wo), np.uint8)
    emul.emul_map(intr.ctypes.data, c["width"], c["height"], pin.ctypes.data, wo, ho, uv.ctypes.data, mask.ctypes.data)
    out = np.full((len(images), ho, wo, 3), 123, np.uint8)
    g = None if gains is None else np.ascontiguousarray(gains, np.int64)
    emul.emul_images(intr.ctypes.data, c["width"], c["height"], pin.ctypes.data, wo, ho, border, len(images),
                     np.ascontiguousarray(images).ctypes.data, None if g is None else g.ctypes.data, out.ctypes.data)
    return uv, mask, out


def all_cases(emul):
    pixels, tw, th, block = host_tile(emul)
    assert pixels * block == tw * th and tw % pixels == 0
    return uc.basic_cases() + uc.tile_cases(pixels, tw, th)


def test_case_conditions(emul):
    """barrel: every pixel valid; border: 5 % .. 95 % invalid; resize: w' h' 3 no multiple of four, batches of 3 and 5; dyadic:
    (i - cx') / fx' exact in float32; tile: each value of the kernel's tile minus one, exact and plus one"""
    cases = all_cases(emul)
    got = {c["name"]: uc.check_conditions(c) for c in cases}
    assert got["barrel"] == 0.0
    assert sum(n.startswith("border") for n in got) == 2
    pixels, tw, th, _ = host_tile(emul)
    sizes = {uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])[1] for c in cases if c["name"].startswith("tile")}
    assert {w for w, _ in sizes} >= {pixels - 1, pixels, pixels + 1, tw - 1, tw, tw + 1} and {h for _, h in sizes} >= {th - 1, th, th + 1}
    assert {uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])[1] for c in cases if c["name"].startswith("resize")} == {(41, 23), (5, 5)}


def test_oracle_matches_the_plain_loops():
    c = uc.case("small", uc.PINCUSHION, 13, 11, m=2, border=9, fx=8.0, fy=9.0, cx=5.25, cy=4.5, out_width=11, out_height=9)
    img, g = uc.images_of(c), uc.gains_of(c)
    uv, mask = uo.position(c["intr"], 13, 11, **c["opts"])
    assert 0 < int((mask == 0).sum()) < mask.size
    for gains in (None, g):
        luv, lmask, lout = uo.loops(img.tolist(), c["intr"], None if gains is None else gains.tolist(), **c["opts"])
        assert np.array(lmask, np.uint8).tolist() == mask.tolist()
        assert np.array(lout, np.uint8).tolist() == uo.images(img, c["intr"], gains, **c["opts"]).tolist()
        for j in range(9):
            for i in range(11):
                if luv[j][i] is None:
                    assert np.isnan(uv[j, i]).all()
                else:
                    assert (float(uv[j, i, 0]), float(uv[j, i, 1])) == luv[j][i]


def test_compiled_header_matches_the_oracle_bit_for_bit(emul):
    for c in all_cases(emul):
        img, g = uc.images_of(c), uc.gains_of(c)
        want_uv, want_mask = uo.position(c["intr"], c["width"], c["height"], **c["opts"])
        for gains in (None, g):
            uv, mask, out = host_run(emul, c, img, gains)
            assert same_bytes(mask, want_mask), c["name"]
            assert np.array_equal(np.isnan(uv), np.isnan(want_uv)) and same_bytes(np.nan_to_num(uv), np.nan_to_num(want_uv)), c["name"]
            assert same_bytes(out, uo.images(img, c["intr"], gains, **c["opts"])), c["name"]


def test_closed_forms_on_the_compiled_header(emul):
    run = lambda c, img, g: host_run(emul, c, img, g)[1:]
    uc.closed_identity(run)
    uc.closed_half_pixel(run)
    uc.closed_constant(run)


def test_closed_forms_on_the_oracle():
    run = lambda c, img, g: (uo.position(c["intr"], c["width"], c["height"], **c["opts"])[1], uo.images(img, c["intr"], g, **c["opts"]))
    uc.closed_identity(run)
    uc.closed_half_pixel(run)
    uc.closed_constant(run)


# ---- the binding and the files
def test_struct_is_48_bytes_and_mirrored(emul, pkg):
    L = pkg._lib
    emul.emul_opts_size.restype = ctypes.c_int
    assert emul.emul_opts_size() == 48 and ctypes.sizeof(L.UndistortOpts) == 48
    assert L.option_names(L.UndistortOpts) == ("fx", "fy", "cx", "cy", "out_width", "out_height", "border", "max_batch_images")
    und = importlib.import_module("global-lvba_amd.undistort")
    assert und.Undistorter._destroy == "lvba_undistort_free" and "lvba_undistort_create" in L.SYMBOLS
    o = und.undistort_opts(border=7)                    # host only: lvba_undistort_default_opts
    assert (o.fx, o.fy, o.cx, o.cy, o.out_width, o.out_height, o.border, o.max_batch_images) == (0.0, 0.0, 0.0, 0.0, 0, 0, 7, 64)
    with pytest.raises(TypeError):
        und.undistort_opts(bordr=1)
    assert und.tile() == host_tile(emul)[:3]


def test_cameras_txt_and_images_txt(tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    ds.write_cameras_txt(tmp_path / "cameras.txt", 41, 29, (64.0, 63.5, 20.5, 14.25))
    assert open(tmp_path / "cameras.txt").read() == "1 PINHOLE 41 29 64.0 63.5 20.5 14.25\n"
    q = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, -0.5, 0.5, 0.5]])
    t = np.array([[0.1, -2.0, 3.0], [1e-7, 2.5, -0.3333333]])
    ds.write_images_txt(tmp_path / "a.txt", q, t)
    want = ("0 1.000000 0.000000 0.000000 0.000000 0.100000 -2.000000 3.000000 1 0.jpg\n0.0 0.0 -1\n"
            "1 0.500000 -0.500000 0.500000 0.500000 0.000000 2.500000 -0.333333 1 1.jpg\n0.0 0.0 -1\n")
    assert open(tmp_path / "a.txt").read() == want      # the default is what it was, byte for byte
    ds.write_images_txt(tmp_path / "b.txt", q, t, ext="png")
    assert open(tmp_path / "b.txt").read() == want.replace(".jpg", ".png")


def test_image_files_round_trip(tmp_path):
    ds = importlib.import_module("global-lvba_amd.dataset")
    img = uc.images_of(uc.basic_cases()[0])[0]
    ds.write_image_bgr(str(tmp_path / "a.png"), img)
    assert same_bytes(ds.read_image_bgr(str(tmp_path / "a.png")), img)              # lossless, and B G R both ways
    smooth = np.stack([np.add.outer(np.arange(29), np.arange(37)) * 3 + 10 * k for k in range(3)], -1).astype(np.uint8)
    ds.write_image_bgr(str(tmp_path / "a.jpg"), smooth)
    back = ds.read_image_bgr(str(tmp_path / "a.jpg"))
    assert back.shape == smooth.shape and np.abs(back.astype(int) - smooth.astype(int)).mean() < 4.0   # JPEG: lossy, the channels in place
    ds.write_image_bgr(str(tmp_path / "m.png"), np.where(img[:, :, 0] > 128, 255, 0).astype(np.uint8))
    assert same_bytes(ds.read_image_bgr(str(tmp_path / "m.png"))[:, :, 1], np.where(img[:, :, 0] > 128, 255, 0).astype(np.uint8))


def test_run_dataset_refusals_need_no_device(tmp_path, monkeypatch):
    """unknown keys, an unknown format, apply_exposure without exposure and a missing out_dir raise ValueError before the dataset
    is read, let alone a device touched"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    monkeypatch.setattr(ds, "load_dataset", lambda *a, **k: pytest.fail("the dataset was read"))
    args = (str(tmp_path), "db.db", uc.BARREL, 37, 29, np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="unknown keys.*focal"):
        pl.run_dataset(*args, out_dir=str(tmp_path / "o"), undistorted_images=dict(focal=3.0))
    with pytest.raises(ValueError, match="format"):
        pl.run_dataset(*args, out_dir=str(tmp_path / "o"), undistorted_images=dict(format="bmp"))
    with pytest.raises(ValueError, match="apply_exposure"):
        pl.run_dataset(*args, out_dir=str(tmp_path / "o"), undistorted_images=dict(apply_exposure=True))
    with pytest.raises(ValueError, match="out_dir"):
        pl.run_dataset(*args, undistorted_images=True)
    assert pl._undistort_request(True, None) == ("jpg", False, {})
    assert pl._undistort_request(dict(format="png", apply_exposure=True, border=5, fx=1.0), True) == ("png", True, dict(border=5, fx=1.0))
