"""The cameras and small random images of the undistort tests (tests/test_undistort_host.py, tests/test_gpu_undistort.py).  A case is
dict(name, intr [8], width, height, opts: lvba_undistort_opts' fields, m: images).  check_conditions asserts on the CPU what each
case is there for, so that no test passes on an empty or a full mask."""
import numpy as np

import undistort_oracle as uo

BARREL = [30.0, 31.0, 18.3, 14.6, -0.2, 0.02, 1e-3, -8e-4]          # 37 x 29: every pixel is pulled inwards
PINCUSHION = [30.0, 31.0, 18.3, 14.6, 0.3, 0.05, 1e-3, -8e-4]       # the rim leaves the image
MILD = [30.0, 31.0, 18.3, 14.6, -0.05, 0.004, 5e-4, 3e-4]
WIDE = [52.0, 50.0, 31.7, 23.4, -0.12, 0.01, 7e-4, -4e-4]           # 64 x 48
DYADIC_PIN = dict(fx=64.0, fy=64.0, cx=20.5, cy=14.25)              # (i - cx) / fx is exact in float32 for every pixel
DYADIC_SRC = [61.0, 63.0, 19.2, 15.1, -0.15, 0.03, 8e-4, -6e-4]     # 40 x 30, distorted


def scaled_pinhole(intr, width, height, wo, ho):
    """the source's pinhole scaled to a wo x ho target"""
    return dict(fx=intr[0] * wo / width, fy=intr[1] * ho / height, cx=intr[2] * wo / width, cy=intr[3] * ho / height,
                out_width=wo, out_height=ho)


def case(name, intr, width, height, m=2, **opts):
    return dict(name=name, intr=np.array(intr, np.float64), width=width, height=height, opts=opts, m=m)


def basic_cases():
    return [
        case("barrel", BARREL, 37, 29),
        case("border_pincushion", PINCUSHION, 37, 29, border=77),
        case("border_short_focal", MILD, 37, 29, fx=14.0, fy=14.5, cx=18.3, cy=14.6, border=200),
        case("resize_41x23_b3", WIDE, 64, 48, m=3, **scaled_pinhole(WIDE, 64, 48, 41, 23)),
        case("resize_41x23_b5", WIDE, 64, 48, m=5, **scaled_pinhole(WIDE, 64, 48, 41, 23)),
        case("resize_5x5_b3", WIDE, 64, 48, m=3, **scaled_pinhole(WIDE, 64, 48, 5, 5)),
        case("resize_5x5_b5", WIDE, 64, 48, m=5, **scaled_pinhole(WIDE, 64, 48, 5, 5)),
        case("dyadic", DYADIC_SRC, 40, 30, out_width=41, out_height=29, **DYADIC_PIN),
    ]


def tile_cases(pixels, tile_w, tile_h):
    """target widths at pixels and tile_w, heights at tile_h, each minus one, exact and plus one"""
    widths = [pixels - 1, pixels, pixels + 1, tile_w - 1, tile_w, tile_w + 1]
    heights = [tile_h - 1, tile_h, tile_h + 1]
    sizes = [(w, heights[k % 3]) for k, w in enumerate(widths)] + [(tile_w + 1, tile_h - 1), (tile_w - 1, tile_h + 1), (pixels + 1, tile_h)]
    return [case(f"tile_{w}x{h}", WIDE, 64, 48, m=3, **scaled_pinhole(WIDE, 64, 48, w, h)) for w, h in sizes]


def images_of(c, seed=5):
    """uint8 [m, height, width, 3]: random bytes, with saturated and black runs so that the clamp and the rounding at 255 are met"""
    rng = np.random.default_rng(seed + c["width"] * 131 + c["m"])
    img = rng.integers(0, 256, (c["m"], c["height"], c["width"], 3), dtype=np.uint8)
    img[:, : c["height"] // 4, : c["width"] // 3] = 255
    img[:, -(c["height"] // 5):, -(c["width"] // 4):] = 0
    return img


def gains_of(c, seed=9):
    """int64 [m, 3, 2]: gains in 0.6 .. 1.7, offsets up to 20 grey levels either way; the first image's reach the clamp"""
    rng = np.random.default_rng(seed + c["m"])
    g = np.zeros((c["m"], 3, 2), np.int64)
    g[:, :, 0] = rng.integers(int(0.6 * 65536), int(1.7 * 65536), (c["m"], 3))
    g[:, :, 1] = rng.integers(-20 * 256 * 65536, 20 * 256 * 65536, (c["m"], 3))
    g[0, 0] = (3 * 65536, 50 * 256 * 65536)
    g[0, 1] = (1 << 14, -60 * 256 * 65536)
    return g


def check_conditions(c):
    """what the case is there for"""
    _, mask = uo.position(c["intr"], c["width"], c["height"], **c["opts"])
    invalid = float((mask == 0).mean())
    (fx, _, cx, _), (wo, ho), _ = uo.resolve(c["intr"], c["width"], c["height"], **c["opts"])
    name = c["name"]
    if name == "barrel":
        assert c["intr"][4] < 0 and (wo, ho) == (37, 29) and invalid == 0.0, invalid
    if name.startswith("border"):
        assert 0.05 <= invalid <= 0.95, invalid
    if name.startswith("resize"):
        assert (wo * ho * 3) % 4 != 0 and c["m"] in (3, 5) and (c["width"], c["height"]) == (64, 48)
    if name == "dyadic":
        i = np.arange(wo, dtype=np.float64)
        x = (i - cx) / fx
        assert (x.astype(np.float32).astype(np.float64) == x).all() and np.any(c["intr"][4:] != 0) and 0.0 < invalid < 0.5
    if name.startswith("tile"):
        assert invalid < 0.5
    return invalid


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- closed forms: no oracle.  run(case, images, gains) -> (mask, out) of the implementation under test
NO_DISTORTION = np.array([64.0, 64.0, 20.5, 14.25, 0.0, 0.0, 0.0, 0.0])


def closed_identity(run):
    """no distortion, the dyadic pinhole, the same size: u = i and v = j exactly, so a valid pixel is its source pixel; the last
    row and column are outside [0, w - 1) x [0, h - 1): border"""
    c = case("identity", NO_DISTORTION, 41, 29, m=2, border=66)
    img = images_of(c)
    mask, out = run(c, img, None)
    want_mask = np.zeros((29, 41), np.uint8)
    want_mask[:-1, :-1] = 255
    assert same_bytes(mask, want_mask)
    assert same_bytes(out[:, :-1, :-1], img[:, :-1, :-1]) and (out[:, -1] == 66).all() and (out[:, :, -1] == 66).all()


def closed_half_pixel(run):
    """cx' moved by exactly 0.5: u = i + 0.5, a = 128, b = 0, so c = 32768 (p0 + p1), c16 = 128 (p0 + p1) and the byte is
    (128 (p0 + p1) + 128) >> 8 = (p0 + p1 + 1) >> 1"""
    c = case("half", NO_DISTORTION, 41, 29, m=2, border=3, fx=64.0, fy=64.0, cx=20.0, cy=14.25)
    img = images_of(c)
    mask, out = run(c, img, None)
    want_mask = np.zeros((29, 41), np.uint8)
    want_mask[:-1, :-1] = 255                            # u = i + 0.5 < 40 for i <= 39
    assert same_bytes(mask, want_mask)
    p = img.astype(np.int64)
    assert same_bytes(out[:, :-1, :-1], ((p[:, :-1, :-1] + p[:, :-1, 1:] + 1) >> 1).astype(np.uint8))
    assert (out[:, -1] == 3).all() and (out[:, :, -1] == 3).all()


def closed_constant(run):
    """a constant image of grey level c under gains (A, B): every valid sample is 256 c, the byte (expo_apply(A, B, 256 c) + 128) >> 8
    with expo_apply on Python integers"""
    c = case("constant", BARREL, 37, 29, m=3, border=1)
    grey = (40, 130, 251)
    img = np.stack([np.full((29, 37, 3), v, np.uint8) for v in grey])
    g = gains_of(c)
    mask, out = run(c, img, g)
    assert (mask == 255).all()
    for q in range(3):
        for k in range(3):
            A, B = int(g[q, k, 0]), int(g[q, k, 1])
            want = (min(max((A * 256 * grey[q] + B + 32768) // 65536, 0), 65280) + 128) >> 8
            assert (out[q, :, :, k] == want).all(), (q, k, want)
    assert len({int(v) for v in out.reshape(-1)}) > 4    # the gains differ: the test is not about one value
