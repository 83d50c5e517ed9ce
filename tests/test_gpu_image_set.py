"""GPU test of the image front ends on ONE image set with empty images (tests/image_set_cases.py): which image a key point belongs
to is csrc/segments.h and the resident key-point table is csrc/image_set.h for all three handles, and every handle is held here
against the oracle its own GPU test uses, with that test's equality -- exact for integers, bit for bit for the lifted points, the
essential matrices and the gathered pixels.

The set: key point counts [0, 1, 0, 0, 65, 40, 0] -- empty images at both ends and two in a row, an image of one key point, an image
longer than a wavefront and than two scan tiles, an image of one tile and a part.  The pair list holds a pair whose first image
is empty, the two full images in both orders, the one-point image, a pair of two empty images and a pair whose first image is
the empty last one.  tests/test_image_set_host.py holds the oracles' results on this set to be non-empty and every fp64 decision
to be at least 1e-9 from its bound, so nothing below can pass on empty arrays or turn on an ulp."""
import importlib

import numpy as np
import pytest

import image_set_cases as ic
import match_depth_oracle as mdo
import verify_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(pkg):
    M = importlib.import_module("global-lvba_amd.match")
    V = importlib.import_module("global-lvba_amd.visual")
    s = ic.image_set()
    with V.DepthImages.upload(s["depth"]) as d, M.Matcher(s["descs"]) as m:
        m.set_geometry(s["keypoints"], s["intr"], s["Rcw"], s["tcw"])
        m.set_depth(d)
        yield m


@pytest.fixture(scope="module")
def verifier(pkg):
    VF = importlib.import_module("global-lvba_amd.verify")
    s = ic.image_set()
    with VF.Verifier(s["keypoints"], s["intr"], Rcw=s["Rcw"]) as v:
        yield v


@pytest.mark.parametrize("guided", (0, 1, 2))
def test_matches_equal_the_oracle(matcher, guided):
    s = ic.image_set()
    wm, ws, woff = ic.oracle_matches(guided)
    matches, scores, off, count = matcher.match_pairs_csr(ic.PAIRS, guided=guided)
    np.testing.assert_array_equal(off, woff)
    assert count == len(wm) >= 33
    np.testing.assert_array_equal(matches, wm)
    np.testing.assert_array_equal(scores, ws)
    for a, b in ic.PAIRS.tolist():
        for x, y in ((a, b), (b, a)):
            for got, want in zip(matcher.scan(x, y, guided=guided), mdo.scan(s["descs"], x, y, ic.geometry(), guided=guided)):
                np.testing.assert_array_equal(got, want, err_msg=f"pair ({x}, {y})")


def test_points_equal_the_oracles_lift(matcher):
    """match_lift_kernel's image of a key point across the runs of empty images: each point goes through ITS image's depth and pose"""
    got, want = matcher.points(), np.concatenate(ic.geometry().points)
    assert got.shape == want.shape == (sum(ic.COUNTS), 3) and np.isfinite(want).all()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("k", range(len(ic.VERIFY_OPTION_SETS)))
def test_verification_equals_the_oracle(verifier, k):
    kw = ic.VERIFY_OPTION_SETS[k]
    put = ic.putative()
    inl, rep = verifier.pairs(ic.VERIFY_PAIRS, put, **kw)
    want = [ic.oracle_verify(p, k) for p in range(len(ic.VERIFY_PAIRS))]
    np.testing.assert_array_equal(rep["status"], [r["status"] for r in want])
    assert rep["status"].tolist() == [vo.OK, vo.OK, vo.TOO_FEW_MATCHES, vo.TOO_FEW_MATCHES]   # the one-match pair, the empty pair
    np.testing.assert_array_equal(rep["best_h"], [r["best_h"] for r in want])
    np.testing.assert_array_equal(rep["n_inliers"], [r["n_inliers"] for r in want])
    np.testing.assert_array_equal(rep["n_matches"], [len(m) for m in put])
    np.testing.assert_array_equal(rep["E"].reshape(-1, 9), np.array([r["E"] for r in want]).reshape(-1, 9))
    for p, (g, r) in enumerate(zip(inl, want)):
        np.testing.assert_array_equal(g, put[p][r["mask"]], err_msg=str(ic.VERIFY_PAIRS[p]))
    s = ic.image_set()
    for p in (0, 1):                                                          # every hypothesis of the two full pairs, bit for bit
        a, b = (int(x) for x in ic.VERIFY_PAIRS[p])
        lo, hi = min(a, b), max(a, b)
        E, count, _ = vo.hypotheses(vo.points(ic.undistorted(), a, b, put[p]), lo, hi, vo.relative_rotation(s["Rcw"][lo], s["Rcw"][hi]),
                                    **dict(vo.DEFAULTS, intr=s["intr"], **kw))
        gE, gcount = verifier.hypotheses(a, b, put[p], **kw)
        np.testing.assert_array_equal(gE.reshape(-1, 9), E)
        np.testing.assert_array_equal(gcount, count)


@pytest.mark.parametrize("thr", ic.THRESHOLDS)
def test_tracks_equal_build_components(pkg, matcher, thr):
    TG = importlib.import_module("global-lvba_amd.trackgraph")
    pl = importlib.import_module("global-lvba_amd.pipeline")
    s = ic.image_set()
    pairs = ic.PAIRS.tolist()
    ms = matcher.match_pairs(ic.PAIRS)                                        # the matcher's own output
    _, comps = pl.match_components(list(ic.COUNTS), pairs, ms, thr)
    want_orders = pl.build_components(list(ic.COUNTS), pairs, ms, thr)
    assert len(comps) >= 1
    flat = [ob for c in comps for ob in c]
    with TG.TrackGraph(s["keypoints"], pairs, ms, obser_thr=thr) as g:
        assert g.info["n_components"] == len(comps) and g.info["n_observations"] == len(flat) and g.info["n_skipped"] == 0
        off, img, kp, images = g.components()
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum([len(c) for c in comps])]))
        np.testing.assert_array_equal(img, [i for i, _ in flat])
        np.testing.assert_array_equal(kp, [k for _, k in flat])
        np.testing.assert_array_equal(images, [len({i for i, _ in c}) for c in comps])
        obs_off, obs_img, obs_kp, obs_uv = g.orders(uv=True)
        for got, want in zip((obs_off, obs_img, obs_kp), want_orders):
            np.testing.assert_array_equal(got, want)
        kp_off = np.concatenate([[0], np.cumsum(ic.COUNTS)])
        assert obs_uv.dtype == np.float32 and obs_uv.tobytes() == np.concatenate(s["keypoints"])[kp_off[obs_img] + obs_kp].tobytes()
