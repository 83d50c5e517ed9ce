"""GPU tests of the depth rendering and the per-track fusion (csrc/fusion.hip, fusion_device.h, tracks_device.h) on the cases of
tests/fusion_cases.py: the rules at their edges, each with expectations derived by hand, and the oracle
(oracle/fusion_oracle.py) on identical inputs.  tests/test_fusion_cases_host.py holds the same cases to the oracle on the CPU
and asserts that no decision in them is within rounding of going the other way.

Depth images: bit for bit (tobytes) -- fusion.hip is built without contraction, both sides draw the smallest (float)Z.
Tracks: status and kept exact, X and mean to 1e-9, dropped rows zeros and +inf (the bars of tests/test_gpu_fusion.py).
Refusals: LVBA_ERR_ARG with every output byte as it was, and the same arguments work once the bad one is mended."""
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import track_oracle as to

import fusion_cases as fc

pytestmark = pytest.mark.gpu

DEPTH = {c["name"]: c for c in fc.depth_cases()}
TRACKS = ("block_edges", "short_and_empty", "image_counts", "bucket_collisions", "long_track", "pixel_edges", "anchor", "selection")


@pytest.fixture(scope="module")
def vis(pkg):
    return importlib.import_module("global-lvba_amd.visual")


def _render(pkg, vis, c):
    with pkg.Scans(c["clouds"]) as scans:
        with vis.DepthImages.render(scans, c["scan_poses"], c["scan_times"], c["image_times"], c["Rcw"], c["tcw"], c["intr"],
                                    c["W"], c["H"], half_window_s=c["half_window"], voxel_size=c["voxel"]) as d:
            assert (d.n_images, d.width, d.height) == (len(c["image_times"]), c["W"], c["H"])
            return np.stack([d.download(m) for m in range(d.n_images)])


@pytest.mark.parametrize("name", sorted(DEPTH))
def test_depth_case(pkg, vis, name):
    c = DEPTH[name]
    want = fc.oracle_depth(c)
    got = _render(pkg, vis, c)
    fc.check_depth_lists(c, got)
    for m in range(len(want)):
        assert got[m].tobytes() == want[m].tobytes(), (name, m, int((got[m] != want[m]).sum()))
    if name in ("one_pixel_contention", "distorted_off_axis"):               # atomicMin: the same image whatever the order
        assert _render(pkg, vis, c).tobytes() == got.tobytes()


def _fuse(vis, c, depth, off=None, img=None, uv=None, **o):
    off, img, uv = (c["off"], c["img"], c["uv"]) if off is None else (off, img, uv)
    return vis.fuse_tracks(off, img, uv, c["Rcw"], c["tcw"], c["intr"], depth=depth, **o)


def _rows_equal(part, whole, tracks, c):
    """The outputs of a call on the tracks `tracks` of c alone against their rows in the call on all of c: the same bytes."""
    for k in range(3):
        assert part[k].tobytes() == whole[k][tracks].tobytes()
    seg = np.concatenate([np.arange(c["off"][t], c["off"][t + 1]) for t in tracks]).astype(np.int64)
    assert part[3].tobytes() == whole[3][seg].tobytes()


@pytest.mark.parametrize("name", TRACKS)
def test_track_case(vis, name):
    c = fc.case_by_name(name)
    with vis.DepthImages.upload(c["depth"]) as d:
        for depth in (d, None):
            got = _fuse(vis, c, depth)
            fc.assert_tracks_match(got, fc.oracle_tracks(c, depth is not None), (name, depth is not None))
            fc.check_track_lists(c, got, depth is not None)
            if name == "block_edges":                                        # a shorter list is the longer one's beginning
                for n in c["prefixes"]:
                    part = _fuse(vis, c, depth, c["off"][:n + 1], c["img"][:c["off"][n]], c["uv"][:c["off"][n]])
                    _rows_equal(part, got, list(range(n)), c)
            if name == "short_and_empty":                                    # no track's result depends on its neighbours
                _rows_equal(_fuse(vis, c, depth, *fc.sub_tracks(c, c["good"])), got, c["good"], c)
            if name == "long_track":
                _rows_equal(_fuse(vis, c, depth, *fc.sub_tracks(c, c["neighbours"])), got, c["neighbours"], c)


@pytest.mark.parametrize("opts", fc.OPTION_SETS, ids=lambda o: "-".join("%s=%g" % kv for kv in o.items()))
def test_options(vis, opts):
    c = fc.case_by_name("options")
    with vis.DepthImages.upload(c["depth"]) as d:
        for depth in (d, None):
            got = _fuse(vis, c, depth, **opts)
            fc.assert_tracks_match(got, fc.oracle_tracks(c, depth is not None, **opts), (opts, depth is not None))


# ------------------------------------------------------------------------------------------------------------- refusals
BAD_OFFSETS = {"decreases": [0, 4, 2, 12], "overshoots_inside": [0, 10, 3, 12], "starts_above_0": [1, 3, 7, 12]}


def _three_tracks():
    """Tracks 0, 4, 5 of image_counts: 3 + 4 + 5 observations, one per image."""
    c = fc.case_by_name("image_counts")
    off, img, uv = fc.sub_tracks(c, [0, 4, 5])
    assert off.tolist() == [0, 3, 7, 12]
    return c, off, img, uv


class _FuseCall:
    """lvba_fuse_tracks itself, with sentinel-filled outputs."""

    def __init__(self, c, img, uv, depth):
        self.L = importlib.import_module("global-lvba_amd._lib")
        self.lib = self.L.load()
        self.c, self.img, self.uv, self.depth = c, np.ascontiguousarray(img), np.ascontiguousarray(uv), depth
        self.R, self.t = np.ascontiguousarray(c["Rcw"]).reshape(-1), np.ascontiguousarray(c["tcw"]).reshape(-1)

    def __call__(self, off, **o):
        n, O = len(off) - 1, len(self.img)
        self.out = (np.full(n, 0xAB, np.uint8), np.full(3 * n, -7.5), np.full(n, -7.5), np.full(O, 0xCD, np.uint8))
        opts = self.L.FuseOpts()
        self.lib.lvba_fuse_default_opts(C.byref(opts))
        for k, v in o.items():
            setattr(opts, k, v)
        st, X, err, kept = self.out
        return self.lib.lvba_fuse_tracks(0, self.depth._h if self.depth is not None else None, len(self.c["Rcw"]), self.R, self.t,
                                         np.ascontiguousarray(self.c["intr"], np.float64), n, np.ascontiguousarray(off, np.int64),
                                         self.img.ctypes.data, self.uv.ctypes.data, C.byref(opts), st.ctypes.data, X, err,
                                         kept.ctypes.data)

    def untouched(self):
        st, X, err, kept = self.out
        return (st == 0xAB).all() and (X == -7.5).all() and (err == -7.5).all() and (kept == 0xCD).all()


def _same_as_oracle(call, c, rc):
    assert rc == 0
    st, X, err, kept = call.out
    want = fc.oracle_tracks(c, call.depth is not None)
    tracks = [0, 4, 5]
    seg = np.concatenate([np.arange(c["off"][t], c["off"][t + 1]) for t in tracks])
    fc.assert_tracks_match((st, X.reshape(-1, 3), err, kept), (want[0][tracks], want[1][tracks], want[2][tracks], want[3][seg]))


@pytest.mark.parametrize("with_depth", (True, False))
def test_fuse_tracks_refuses_bad_offsets_and_options(vis, with_depth):
    c, off, img, uv = _three_tracks()
    with vis.DepthImages.upload(c["depth"]) as d:
        call = _FuseCall(c, img, uv, d if with_depth else None)
        for what, bad in BAD_OFFSETS.items():
            assert call(np.array(bad, np.int64)) == call.L.ERR_ARG and call.untouched(), what
        _same_as_oracle(call, c, call(off))
        for o in (dict(obser_thr=0), dict(obser_thr=-1), dict(min_view_angle_deg=np.nan), dict(min_view_angle_deg=-1.0),
                  dict(min_view_angle_deg=180.5), dict(min_view_angle_deg=np.inf), dict(reproj_mean_thr_px=np.nan),
                  dict(reproj_mean_thr_px=-1.0)):
            assert call(off, **o) == call.L.ERR_ARG and call.untouched(), o
        _same_as_oracle(call, c, call(off))
        # the bounds themselves are options like any other
        assert call(off, obser_thr=1, min_view_angle_deg=0.0, reproj_mean_thr_px=0.0) == 0
        assert call(off, min_view_angle_deg=180.0, reproj_mean_thr_px=np.inf) == 0


def test_triangulate_tracks_refuses_bad_offsets(pkg):
    c, off, img, uv = _three_tracks()
    L = importlib.import_module("global-lvba_amd._lib")
    lib = L.load()
    uv64 = np.ascontiguousarray(uv, np.float64)
    R, t = np.ascontiguousarray(c["Rcw"]).reshape(-1), np.ascontiguousarray(c["tcw"]).reshape(-1)

    def call(o):
        out = (np.full(9, -7.5), np.full(3, -7.5), np.full(3, -77, np.int32), np.full(3, 0xAB, np.uint8))
        rc = lib.lvba_triangulate_tracks(0, len(c["Rcw"]), 3, np.ascontiguousarray(o, np.int64), img.ctypes.data, uv64.ctypes.data, R, t,
                                         np.ascontiguousarray(c["intr"], np.float64), *out)
        return rc, out
    for what, bad in BAD_OFFSETS.items():
        rc, (X, err, cnt, ok) = call(bad)
        assert rc == L.ERR_ARG and (X == -7.5).all() and (err == -7.5).all() and (cnt == -77).all() and (ok == 0xAB).all(), what
    rc, (X, err, cnt, ok) = call(off)
    assert rc == 0
    ok_o, X_o, err_o, cnt_o = to.triangulate_tracks(c["intr"], c["Rcw"], c["tcw"], off, img, uv64)
    assert ok.tolist() == ok_o.tolist() == [0, 1, 1] and cnt[1:].tolist() == cnt_o[1:].tolist()
    assert np.abs(X.reshape(3, 3)[1:] - X_o[1:]).max() <= 1e-8 and np.abs(err[1:] - err_o[1:]).max() <= 1e-8
