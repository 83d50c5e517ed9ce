"""CPU test of the image-set fixture (tests/image_set_cases.py): what the case claims, so that tests/test_gpu_image_set.py cannot
pass on empty results -- the counts and what images 1, 4 and 5 share, the margin of every fp64 decision of the oracles, at least
33 matches for (4, 5), the verify oracle's OK for it, the statuses of the one-match and the empty pair, tracks under both
thresholds -- and the Python helper that flattens per-image arrays for the three wrappers."""
import importlib

import numpy as np
import pytest

import image_set_cases as ic
import match_cases as mc
import verify_oracle as vo


def test_the_case_is_what_it_says():
    s = ic.image_set()
    assert tuple(len(k) for k in s["keypoints"]) == tuple(len(d) for d in s["descs"]) == ic.COUNTS == (0, 1, 0, 0, 65, 40, 0)
    assert all(k.dtype == np.float32 and k.shape[1:] == (2,) for k in s["keypoints"])
    l1, l4, l5 = (s["landmark"][v] for v in (1, 4, 5))
    shared = set(l4[l4 >= 0]) & set(l5[l5 >= 0])
    assert len(shared) >= 33 and l1.tolist()[0] in shared
    assert ic.COUNTS[4] > 64 and ic.COUNTS[4] > 2 * 32 and 32 < ic.COUNTS[5] < 64     # a wavefront, two scan tiles; a tile and a part
    assert s["depth"].shape[0] == len(ic.COUNTS) and (s["depth"] > 0).all()             # the lift is defined everywhere


def test_every_decision_keeps_its_margin():
    worst = ic.check_margins()
    print("smallest margin of any matcher decision:", worst)
    assert worst >= mc.MIN_MARGIN
    hyp = ic.hypothesis_margin()
    print("smallest relative margin of any (pair, hypothesis, match) of the verifier:", hyp)
    assert hyp >= 1e-9


@pytest.mark.parametrize("guided", (0, 1, 2))
def test_the_oracle_matcher_keeps_the_shared_landmarks(guided):
    s = ic.image_set()
    matches, scores, off = ic.oracle_matches(guided)
    assert len(off) == len(ic.PAIRS) + 1 and off[-1] == len(matches) == len(scores)
    p = ic.PAIRS.tolist().index([4, 5])
    m45 = matches[off[p]:off[p + 1]]
    assert len(m45) >= 33
    assert (s["landmark"][4][m45[:, 0]] == s["landmark"][5][m45[:, 1]]).all() and (s["landmark"][4][m45[:, 0]] >= 0).all()
    n = np.diff(off)
    assert n[ic.PAIRS.tolist().index([1, 4])] == 1                                      # image 1's key point finds its landmark in 4
    assert n[ic.PAIRS.tolist().index([0, 4])] == n[ic.PAIRS.tolist().index([2, 3])] == n[ic.PAIRS.tolist().index([6, 5])] == 0


def test_the_lift_is_defined():
    pts = np.concatenate(ic.geometry().points)
    assert pts.shape == (sum(ic.COUNTS), 3) and np.isfinite(pts).all()


@pytest.mark.parametrize("k", range(len(ic.VERIFY_OPTION_SETS)))
def test_the_verify_oracle_reports_ok_for_4_5(k):
    want = {(4, 5): vo.OK, (5, 4): vo.OK, (1, 4): vo.TOO_FEW_MATCHES, (0, 4): vo.TOO_FEW_MATCHES}
    for p, (a, b) in enumerate(ic.VERIFY_PAIRS.tolist()):
        r = ic.oracle_verify(p, k)
        assert r["status"] == want[(a, b)], (a, b, r["status"])
        if r["status"] == vo.OK:
            assert r["n_inliers"] >= 33 and r["mask"].sum() == r["n_inliers"] and r["best_h"] >= 0
    assert [len(m) for m in ic.putative()] == [len(ic.putative()[0]), len(ic.putative()[0]), 1, 0]


def test_the_tracks_are_not_empty():
    pl = importlib.import_module("global-lvba_amd.pipeline")
    matches, _, off = ic.oracle_matches(0)
    ms = [matches[off[p]:off[p + 1]] for p in range(len(ic.PAIRS))]
    n2 = len(pl.build_components(list(ic.COUNTS), ic.PAIRS.tolist(), ms, 2)[0]) - 1
    o3, img3, _ = pl.build_components(list(ic.COUNTS), ic.PAIRS.tolist(), ms, 3)
    assert n2 >= 33 and len(o3) - 1 >= 1 and sorted(img3[:3].tolist()) == [1, 4, 5]   # the landmark that images 1, 4 and 5 share


def test_flatten_rows():
    L = importlib.import_module("global-lvba_amd._lib")
    flat, off = L.flatten_rows([np.zeros((0, 2)), [[1, 2], [3, 4]], [], [(5, 6)]], np.float32, 2)
    assert flat.dtype == np.float32 and flat.flags.c_contiguous and flat.tolist() == [[1, 2], [3, 4], [5, 6]]
    assert off.dtype == np.int64 and off.tolist() == [0, 0, 2, 2, 3]
    flat, off = L.flatten_rows([], np.uint8, 128)
    assert flat.shape == (0, 128) and flat.dtype == np.uint8 and off.tolist() == [0]
    flat, off = L.flatten_rows([np.arange(4)], np.int32, 2)                              # each array is taken as rows of `width`
    assert flat.tolist() == [[0, 1], [2, 3]] and off.tolist() == [0, 2]
