"""GPU tests of the SIFT extractor (lvba_sift_*, features.py) against the numpy restatement (tests/sift_oracle.py) on the seeded
images of tests/sift_cases.py.  The pyramid and the refined candidates are compared bit for bit; orientations and
descriptors bit for bit on every key point that the oracle's own 1e-12 perturbation leaves alone (test_sift_host.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import match_oracle as mo
import sift_cases as sc
import sift_oracle as so
from test_sift_host import MAX_FRAGILE_SHARE, ORI_TOL, WARP_MATCH_FLOOR, warp_share

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ft(pkg):
    return importlib.import_module("global-lvba_amd.features")


def pyramid_cases(T):
    """(image, options): both odd sizes (the halving rule), a top octave 8 wide (blur radius > width), a single octave, and
    widths at the blur kernel's tile width -- in the first octave with first_octave = 0, in the second with -1"""
    out = []
    for fo in (-1, 0):
        out += [(sc.image(96, 80, 1, grey=(fo == 0)), dict(first_octave=fo)), (sc.image(61, 47, 2, grey=(fo == -1)), dict(first_octave=fo)),
                (sc.image(16, 16, 4), dict(first_octave=fo))]
        for k, w in enumerate((T - 1, T, T + 1)):
            out.append((sc.image(w, 21, 20 + k, grey=bool(k & 1)), dict(first_octave=fo)))
    out.append((sc.image(8, 8, 5), dict(first_octave=0)))
    return out


def test_pyramid_bit_for_bit(ft):
    T = ft.tile_width()
    for img, opts in pyramid_cases(T):
        o = so.options(**opts)
        pyr = so.pyramid(img, o, sc.library_taps(**opts))
        h, w = img.shape[:2]
        assert [(G.shape[2], G.shape[1]) for G, _ in pyr] == so.octave_sizes(w, h, o)
        for k, (G, D) in enumerate(pyr):
            g, d = ft.pyramid(img, o["first_octave"] + k, **opts)
            np.testing.assert_array_equal(g, G, err_msg=f"{w} x {h} {opts} octave {k}: Gaussian levels")
            np.testing.assert_array_equal(d, D, err_msg=f"{w} x {h} {opts} octave {k}: DoG levels")
    assert len(so.octave_sizes(8, 8, so.options(first_octave=0))) == 1 and so.octave_sizes(16, 16, so.options())[-1] == (8, 8)


def test_candidates_exactly(ft):
    T = ft.tile_width()
    cases = pyramid_cases(T) + [(sc.constant(20, 16), {}), (sc.border_extremum(), dict(first_octave=0))]
    total = 0
    for img, opts in cases:
        o = so.options(**opts)
        want = so.candidates(so.pyramid(img, o, sc.library_taps(**opts)), o)
        xys, where, count = ft.candidates(img, **opts)
        assert count == len(want) == len(xys), (img.shape, opts)
        if want:
            np.testing.assert_array_equal(where, np.array([(c["octave"], c["l"]) for c in want], np.int32))
            assert xys.tobytes() == np.stack([c["xys"] for c in want]).tobytes()
        total += len(want)
    assert total > 100
    assert ft.candidates(sc.constant(20, 16))[2] == 0 and ft.candidates(sc.border_extremum(), first_octave=0)[2] == 0


def check_features(kp, ds, count, ref, max_ori):
    """the rows of one image against the oracle's result with its fragility mask"""
    assert float(ref["fragile"].mean()) <= MAX_FRAGILE_SHARE
    p = 0
    for c, feats, fragile in zip(ref["candidates"], ref["features"], ref["fragile"]):
        if fragile:
            n = 0
            while p + n < len(kp) and n < max_ori and kp[p + n, :3].tobytes() == c["xys"].tobytes():
                n += 1
            p += n
            continue
        for theta, b in feats:
            assert kp[p, :3].tobytes() == c["xys"].tobytes()
            d = abs(float(kp[p, 3]) - float(theta))
            assert min(d, so.TWO_PI - d) <= ORI_TOL
            np.testing.assert_array_equal(ds[p], b)
            p += 1
    assert p == len(kp) == count


def test_features_equal_the_oracle(ft):
    for name, _, _ in sc.FEATURE_CASES:
        img, opts, ref = sc.reference(name)
        kp, ds, counts = ft.extract([img], **opts)
        assert kp[0].dtype == np.float32 and ds[0].dtype == np.uint8 and ds[0].shape[1] == 128
        check_features(kp[0], ds[0], int(counts[0]), ref, 2)
        if not ref["fragile"].any():
            assert kp[0][:, :3].tobytes() == ref["keypoints"][:, :3].tobytes() and int(counts[0]) == ref["count"]


def test_batching_gives_the_same_bytes(ft):
    imgs = [sc.image(70, 52, 30 + k) for k in range(5)]
    alone = [ft.extract([im]) for im in imgs]
    want = [(a[0][0].tobytes(), a[1][0].tobytes(), int(a[2][0])) for a in alone]
    assert all(w[2] > 10 for w in want)

    def run(which, **kw):
        kp, ds, counts = ft.extract([imgs[k] for k in which], **kw)
        return [(kp[n].tobytes(), ds[n].tobytes(), int(counts[n])) for n in range(len(which))]
    for m in (1, 3, 5):
        for chunk in (1, 2, 0):
            assert run(range(m), chunk_images=chunk) == want[:m], (m, chunk)
    assert run(range(4, -1, -1), chunk_images=2) == want[::-1]
    assert run(range(5)) == run(range(5))


def test_caps(ft):
    img, opts, ref = sc.reference("bgr_96x80")
    # max_features below the true count: the largest sigma, in canonical order
    o = so.options(max_features=20)
    kp_w, ds_w, count_w, _ = so.assemble(ref["candidates"], ref["features"], o)
    kp, ds, counts = ft.extract([img], max_features=20)
    assert int(counts[0]) == count_w == ref["count"] > 20 and len(kp[0]) == 20
    assert kp[0][:, :3].tobytes() == kp_w[:, :3].tobytes()
    np.testing.assert_array_equal(ds[0], ds_w)
    # capacity below the total: only the first rows are written, the counts and offsets are the true ones
    other = sc.image(96, 80, 7)
    full_kp, full_ds, full_counts = ft.extract([img, other])
    lib = importlib.import_module("global-lvba_amd._lib").load()
    cap = ref["count"] + 5
    a = np.ascontiguousarray(np.stack([img, other]))
    kpb = np.full((cap + 3, 4), -7.0, np.float32)
    dsb = np.full((cap + 3, 128), 0xAB, np.uint8)
    off, cnt = np.zeros(3, np.int64), np.zeros(2, np.int64)
    assert lib.lvba_sift_extract(0, 2, 96, 80, 3, a.ctypes.data, None, cap, off.ctypes.data, kpb.ctypes.data, dsb.ctypes.data,
                                 cnt.ctypes.data) == 0
    assert list(cnt) == [int(c) for c in full_counts] and list(off) == [0, len(full_kp[0]), len(full_kp[0]) + len(full_kp[1])]
    assert off[2] > cap
    assert kpb[:cap].tobytes() == np.concatenate(full_kp)[:cap].tobytes() and dsb[:cap].tobytes() == np.concatenate(full_ds)[:cap].tobytes()
    assert (kpb[cap:] == -7.0).all() and (dsb[cap:] == 0xAB).all()
    kp2, ds2, _ = ft.extract([img, other], capacity=cap)
    assert len(kp2[0]) == len(full_kp[0]) and len(kp2[1]) == 5
    # one orientation per key point
    o1 = so.options(max_orientations=1)
    feats1 = so.describe(ref["pyramid"], ref["candidates"], o1)
    kp_1, ds_1, count_1, _ = so.assemble(ref["candidates"], feats1, o1)
    kp, ds, counts = ft.extract([img], max_orientations=1)
    assert int(counts[0]) == count_1 == sum(min(1, len(f)) for f in ref["features"]) < ref["count"]
    assert kp[0][:, :3].tobytes() == kp_1[:, :3].tobytes()
    np.testing.assert_array_equal(ds[0], ds_1)
    np.testing.assert_array_equal(kp[0][:, 3], kp_1[:, 3])


def test_refusals_write_nothing(ft):
    """NULL arguments, sizes, channels and every option out of range: LVBA_ERR_ARG, the outputs untouched, and the refusal comes
    before a device is looked for (device 99 does not exist: the message is about the argument)."""
    L = importlib.import_module("global-lvba_amd._lib")
    lib = L.load()
    img = np.ascontiguousarray(sc.image(24, 20, 1))
    kp = np.full((64, 4), -7.0, np.float32)
    ds = np.full((64, 128), 0xAB, np.uint8)
    off, cnt = np.full(2, -5, np.int64), np.full(1, -5, np.int64)

    def call(device=99, n=1, w=24, h=20, ch=3, im=img.ctypes.data, opts=None, cap=64, off_p=off.ctypes.data, kp_p=kp.ctypes.data,
             ds_p=ds.ctypes.data, cnt_p=cnt.ctypes.data):
        return lib.lvba_sift_extract(device, n, w, h, ch, im, C.byref(opts) if opts is not None else None, cap, off_p, kp_p, ds_p, cnt_p)
    bad_calls = [dict(im=None), dict(off_p=None), dict(kp_p=None), dict(ds_p=None), dict(cnt_p=None), dict(n=-1), dict(cap=-1),
                 dict(w=7), dict(h=7), dict(ch=2), dict(ch=4), dict(w=20000)]
    for name, values in (("first_octave", (-2, 1)), ("n_intervals", (1, 6)), ("sigma0", (1.0, 4.5, float("nan"))),
                         ("dog_threshold", (0.0, -0.01, 1.5, float("inf"))), ("edge_threshold", (0.5, float("nan"))),
                         ("orientation_window", (0.0, 7.0)), ("max_orientations", (0, 5)), ("max_features", (0, -3)),
                         ("chunk_images", (-1,))):
        for v in values:
            bad_calls.append(dict(opts=ft.sift_opts(**{name: v})))
    o = ft.sift_opts()
    o.reserved = 1
    bad_calls.append(dict(opts=o))
    for kw in bad_calls:
        assert call(**kw) == L.ERR_ARG, kw
        assert b"device" not in lib.lvba_last_error()[:12]
        assert (kp == -7.0).all() and (ds == 0xAB).all() and (off == -5).all() and (cnt == -5).all()
    assert call(device=99) == L.ERR_ARG and b"device" in lib.lvba_last_error()             # a good call, no such device
    assert (kp == -7.0).all() and (off == -5).all()
    g, d = np.full((6, 20, 24), -7.0, np.float32), np.full((5, 20, 24), -7.0, np.float32)
    for kw in (dict(octave=-2), dict(octave=3), dict(w=7), dict(ch=2), dict(im=None)):
        args = dict(w=24, h=20, ch=3, im=img.ctypes.data, octave=0)
        args.update(kw)
        assert lib.lvba_sift_pyramid(99, args["w"], args["h"], args["ch"], args["im"], None, args["octave"], g.ctypes.data,
                                     d.ctypes.data) == L.ERR_ARG
        assert (g == -7.0).all() and (d == -7.0).all()
    n = C.c_int64(-5)
    assert lib.lvba_sift_candidates(99, 24, 20, 2, img.ctypes.data, None, 64, kp.ctypes.data, off.ctypes.data, C.byref(n)) == L.ERR_ARG
    assert n.value == -5
    with pytest.raises(ValueError):
        ft.extract([img, img[:10]])
    with pytest.raises(TypeError):
        ft.extract([img], octaves=3)


def test_end_to_end_through_the_matcher(ft):
    """A texture and its warp by a known similarity: the GPU's features through the GPU matcher give the matches that the oracle's
    features give through the matcher's oracle, and at least WARP_MATCH_FLOOR of them lie within 2 px of the similarity -- the
    descriptors mean to the matcher what the database's did (origin, angle sign, bin order, the factor 512)."""
    M = importlib.import_module("global-lvba_amd.match")
    imgs, want = sc.warp_reference()
    kp, ds, counts = ft.extract(list(imgs))
    with M.Matcher(ds) as m:
        got = m.match_pairs([(0, 1)])[0]
    ref, _ = mo.match_pair([want[0][1], want[1][1]], 0, 1)
    np.testing.assert_array_equal(got, ref)
    share, n = warp_share(kp[0], kp[1], got)
    print(f"warp pair on the device: {[len(k) for k in kp]} features, {n} matches, share within 2 px {share:.4f}")
    assert n >= 50 and share >= WARP_MATCH_FLOOR
