"""CPU tests of the descriptor matcher's depth-guided gate (include/lvba_hip.h "Depth-guided gate"): the numpy
oracle against the rule as plain loops, the symmetry of the two orientations, the device header compiled for the host against
the oracle bit for bit, the fixture's conditions (margins, branches, special keypoints), and the claim -- textures that repeat
along the epipolar line defeat the epipolar gate and come back under the depth gate."""
import ctypes

import numpy as np
import pytest

import match_cases as mc
import match_depth_cases as mdc
import match_depth_oracle as mdo
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/match_device.h compiled for the host, without contraction (tests/match_depth_check.cpp)"""
    lib = ctypes.CDLL(build_check("match_depth_check", tmp_path_factory.mktemp("emul_match_depth")))
    P = ctypes.c_void_p
    lib.emul_lift.argtypes = [ctypes.c_int64, P, P, P, ctypes.c_int, ctypes.c_int, P, P, P]
    lib.emul_predict.argtypes = [ctypes.c_int64, P, P, P, P, P]
    lib.emul_scan_depth.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, P, ctypes.c_double, P, P, P]
    for f in (lib.emul_lift, lib.emul_predict, lib.emul_scan_depth):
        f.restype = None
    return lib


def ptr(x):
    return x.ctypes.data


def host_points(emul, f, geo, i):
    uv = np.ascontiguousarray(f["keypoints"][i], np.float32)
    xy, img = np.ascontiguousarray(geo.xy[i]), np.ascontiguousarray(f["depth"][i])
    out = np.zeros((max(len(uv), 1), 3))
    emul.emul_lift(len(uv), ptr(uv), ptr(xy), ptr(img), img.shape[1], img.shape[0], ptr(np.ascontiguousarray(geo.R[i])),
                   ptr(np.ascontiguousarray(geo.t[i])), ptr(out))
    return out[:len(uv)]


def host_predictions(emul, geo, a, b):
    X = np.ascontiguousarray(geo.points[a])
    out = np.zeros((max(len(X), 1), 2))
    emul.emul_predict(len(X), ptr(geo.intr), ptr(np.ascontiguousarray(geo.R[b])), ptr(np.ascontiguousarray(geo.t[b])), ptr(X), ptr(out))
    return out[:len(X)]


def host_scan(emul, f, geo, a, b, px):
    A, B = f["descs"][a], f["descs"][b]
    ua, ub = (np.ascontiguousarray(f["keypoints"][i], np.float32) for i in (a, b))
    pa, pb = np.ascontiguousarray(geo.predictions(a, b)), np.ascontiguousarray(geo.predictions(b, a))
    best, s1, s2 = (np.zeros(max(len(A), 1), np.int32) for _ in range(3))
    emul.emul_scan_depth(len(A), len(B), ptr(A), ptr(B), ptr(ua), ptr(ub), ptr(pa), ptr(pb), float(px) * float(px), ptr(best), ptr(s1), ptr(s2))
    return best[:len(A)], s1[:len(A)], s2[:len(A)]


def test_oracle_mask_equals_the_rule_as_loops():
    """a tiny case that holds every kind of keypoint: with a point, in a hole, on the hole's edge, the pole (nowhere in view 4) and
    the NaN pixel"""
    f, geo = mdc.facade(), mdc.geometry()
    for a, b, px in ((0, 4, 8.0), (4, 0, 8.0), (3, 1, 3.0), (1, 3, 8.0), (5, 0, 8.0), (0, 5, 3.0), (6, 3, 8.0), (3, 6, 8.0), (4, 3, 8.0)):
        np.testing.assert_array_equal(geo.depth_mask(a, b, px), mdo.loops_mask(geo, a, b, px), err_msg=f"pair ({a}, {b})")


def test_both_orientations_take_the_same_decision():
    geo = mdc.geometry()
    for a, b in mdc.PAIRS:
        for px in (3.0, 8.0):
            np.testing.assert_array_equal(geo.depth_mask(int(a), int(b), px), geo.depth_mask(int(b), int(a), px).T)


def test_device_header_on_the_host_equals_the_oracle(emul):
    """the lifting, the predictions and the scan's (best, s1, s2) of both orientations, bit for bit"""
    f = mdc.facade()
    for second in (False, True):
        geo = mdc.geometry(second)
        for i in range(len(mdc.COUNTS)):
            np.testing.assert_array_equal(host_points(emul, f, geo, i), geo.points[i], err_msg=f"image {i}")
        for a, b in mdc.PAIRS if not second else mdc.PAIRS[:3]:
            for x, y in ((int(a), int(b)), (int(b), int(a))):
                np.testing.assert_array_equal(host_predictions(emul, geo, x, y), geo.predictions(x, y), err_msg=f"pair ({x}, {y})")
                for px in (8.0, 3.0):
                    for got, want in zip(host_scan(emul, f, geo, x, y, px), mdo.scan(f["descs"], x, y, geo, guided=2, max_reproj_px=px)):
                        np.testing.assert_array_equal(got, want, err_msg=f"pair ({x}, {y}) at {px} px")


def test_fixture_conditions():
    f, geo = mdc.facade(), mdc.geometry()
    assert tuple(len(d) for d in f["descs"]) == mdc.COUNTS == tuple(len(k) for k in f["keypoints"])
    # the margin condition, for every option set the GPU tests use
    assert mdc.check_margins(f["descs"], mdc.PAIRS, mdc.DEPTH_OPTION_SETS + (dict(guided=1), dict(guided=0)), geo) >= mc.MIN_MARGIN
    assert mdc.check_margins(f["descs"], mdc.PAIRS, mdc.DEPTH_OPTION_SETS[:1], mdc.geometry(second=True)) >= mc.MIN_MARGIN
    # every branch of the rule occurs in a tested pair
    for a, b in mdc.HORIZONTAL[:1]:
        assert all(n > 0 for n in geo.branches(a, b)), geo.branches(a, b)
    # the special keypoints
    (i, k) = f["special"]["nan"]
    assert np.isnan(f["keypoints"][i][k]).all() and np.isnan(geo.points[i][k]).all()
    assert not geo.depth_mask(i, 0, 8.0)[k].any() and not geo.depth_mask(0, i, 8.0)[:, k].any()   # no distance to it: it takes nothing
    (i, k) = f["special"]["pole"]
    assert np.isfinite(geo.points[i][k]).all() and abs(geo.points[i][k][2] - mdc.POLE[4]) < 1e-6
    assert np.isinf(geo.predictions(i, 4)[k]).all() and not geo.depth_mask(i, 4, 8.0)[k].any()
    assert np.isfinite(geo.predictions(i, 1)[k]).all()
    (i, k) = f["special"]["edge"]
    u, v = f["keypoints"][i][k]
    nb = f["depth"][i][int(v):int(v) + 2, int(u):int(u) + 2]
    assert (nb > 0).sum() == 3 and np.isnan(geo.points[i][k]).all()
    # the lifted points are the planted ones (bilinear depth on a slanted plane, 0.3 px of keypoint noise)
    for i in range(4):
        has = (f["point"][i] >= 0) & ~np.isnan(geo.points[i][:, 0])
        assert has.sum() >= 20 and np.abs(geo.points[i][has] - f["X"][f["point"][i][has]]).max() < 0.03


def test_depth_gate_recovers_textures_repeated_along_the_epipolar_line():
    f, geo = mdc.facade(), mdc.geometry()
    for px in (8.0, 3.0):
        for a, b in mdc.HORIZONTAL:
            for x, y in ((a, b), (b, a)):
                rep, uniq = mc.planted_matches(f, x, y, True), mc.planted_matches(f, x, y, False)
                assert len(rep) >= 55
                epi = set(map(tuple, mdo.match_pair(f["descs"], x, y, geo, guided=1, max_epipolar_px=4.0)[0].tolist()))
                assert not epi & rep                                                    # the copies lie along the line
                got = set(map(tuple, mdo.match_pair(f["descs"], x, y, geo, guided=2, max_reproj_px=px)[0].tolist()))
                hp, hq = ~np.isnan(geo.points[x][:, 0]), ~np.isnan(geo.points[y][:, 0])
                reachable = {(r, c) for r, c in rep | uniq if hp[r] or hq[c]}
                assert reachable <= got, sorted(reachable - got)                        # every planted match with a point
                assert not got - rep - uniq                                             # nothing wrong
                assert not {(r, c) for r, c in got if not (hp[r] or hq[c])}             # nothing where neither has a point
                assert len(reachable & rep) >= 40
                if (a, b) == (0, 1):                                                    # both views have a hole, overlapping in part
                    assert len((rep | uniq) - reachable) > 0 and len({(r, c) for r, c in reachable if hp[r] != hq[c]}) > 0
