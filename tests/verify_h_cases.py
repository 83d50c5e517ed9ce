"""Fixtures of the homography model's tests (tests/test_verify_h_host.py on the CPU, tests/test_gpu_verify_h.py on the GPU), on
verify_cases' two scenes: the planted claims on the plane at 30 %, 60 % and 80 % outliers and in general position, the match-count
ladder either side of the sample size, the wavefront and the LDS chunk, H either side of the hypothesis block, one match repeated,
four matches of which three are collinear in lo, and a mixed batch of about 40 pairs, planar and general together, on a third
scene that holds the images of both (general 0 .. 3, planar 4 .. 7) so that one call can see both kinds.

The collinear case needs three keypoints EXACTLY on a line after undistortion, which no keypoint of a distorted camera is: it has
a two-image scene of its own with zero distortion and pixel coordinates that are dyadic rationals.

verify_cases' match lists let a wrong match land on a keypoint another match uses; two sample points on one keypoint give an H
that is singular in exact arithmetic, for which no margin can hold.  Every list here is thinned to distinct keypoints
(`distinct`), and the claims' lists are topped up to the length and the share of outliers they had (`same_share`).

Margin condition: as verify_cases', and on top of the two distance tests it covers p2 > 0, q2 > 0, the sign at the first sample
point and det H != 0, each scaled by the terms it is a sum of (verify_h_oracle)."""
import functools

import numpy as np

import match_oracle as mo
import verify_cases as vc
import verify_h_oracle as ho
import verify_oracle as vo

MIN_MARGIN = vc.MIN_MARGIN
SIZES = (0, 3, 4, 5, 63, 64, 65, vc.CHUNK - 1, vc.CHUNK, vc.CHUNK + 1)
H_SMALL, H_EDGES = vc.H_SMALL, vc.H_EDGES
PLANAR_OFFSET = 4                # the planar scene's images in the scene of both
PLANAR_80_SEED = 7               # at 80 % one hypothesis in 600 is all planted: the third draw of default_rng(5) has none among its 1024
TOP_UP_SEED = 11
GENERAL_NAN_SEED = 6           # verify_cases' own general-30%-nan, thinned to distinct keypoints, lets E take one wrong match in


def _case(sc, name, a, b, matches, planted, **opts):
    return dict(vc._case(sc, name, a, b, matches, planted, **opts), scene=sc)


def distinct(matches, planted, m=None):
    """(matches, planted) without the wrong matches that share a keypoint of either image with a planted match or with an earlier
    wrong one, cut to the first m rows.  Two sample points on one keypoint make H singular in exact arithmetic: its det and a p2
    are then rounding noise around 0, which no margin condition can hold.  Planted matches are distinct by construction."""
    seen = [set(matches[planted, 0].tolist()), set(matches[planted, 1].tolist())]
    keep = planted.copy()
    for i in np.flatnonzero(~planted):
        a, b = (int(x) for x in matches[i])
        if a not in seen[0] and b not in seen[1]:
            keep[i] = True
            seen[0].add(a); seen[1].add(b)
    mm, pl = np.ascontiguousarray(matches[keep]), planted[keep]
    if m is not None:
        assert len(mm) >= m, (len(mm), m)
        mm, pl = np.ascontiguousarray(mm[:m]), pl[:m]
    return mm, pl


def same_share(sc, a, b, matches, planted, rng):
    """distinct(matches, planted) topped up with further wrong matches on unused keypoints (drawn by verify_cases' generator, so
    each is >= 20 px off its epipolar line in both images) until the list has the length and the share of outliers it had"""
    mm, pl = distinct(matches, planted)
    need = len(matches) - len(mm)
    if need > 0:
        extra, _ = vc.make_matches(sc, a, b, 4 * need + 50, 1.0, rng)
        mm, pl = distinct(np.concatenate([mm, extra]), np.concatenate([pl, np.zeros(len(extra), bool)]), m=len(matches))
    assert len(mm) == len(matches) and pl.sum() == planted.sum()
    return mm, pl


def make_distinct(sc, a, b, m, share, rng, with_nan=False):
    """m matches of distinct keypoints with about `share` of them wrong: half as many again are drawn, then cut to m"""
    return distinct(*vc.make_matches(sc, a, b, m + m // 2 + 2 if m else 0, share, rng, with_nan=with_nan), m=m)


@functools.lru_cache(None)
def both():
    """the images of the general scene (0 .. 3) and of the planar scene (4 .. 7) as one scene"""
    g, p = vc.general()["scene"], vc.planar()["scene"]
    return dict(keypoints=g["keypoints"] + p["keypoints"], xy=g["xy"] + p["xy"], intr=g["intr"], Rcw=np.concatenate([g["Rcw"], p["Rcw"]]),
                tcw=np.concatenate([g["tcw"], p["tcw"]]), rng_seed=(g["rng_seed"], p["rng_seed"]))


@functools.lru_cache(None)
def collinear_scene():
    """two images without distortion; keypoints 0, 1, 2 of either image are exactly collinear after undistortion, 3 is off the line"""
    intr = np.array([512.0, 512.0, 320.0, 256.0, 0.0, 0.0, 0.0, 0.0])
    k0 = np.array([[320 + 64, 256 + 32], [320 + 128, 256 + 64], [320 - 192, 256 - 96], [320 + 40, 256 - 130]], np.float32)
    k1 = k0 + np.array([-96, 24], np.float32)      # a plane carries a line to a line: the matches of the three are collinear too
    k1[3] = (130, 350)
    kps = [k0, k1]
    return dict(keypoints=kps, xy=[mo.undistort_all(intr, k) for k in kps], intr=intr, Rcw=np.stack([np.eye(3)] * 2), tcw=np.zeros((2, 3)),
                rng_seed=-1)


@functools.lru_cache(None)
def cases():
    """dict(planar_claims, general_claims, sizes, h_edges, special, collinear, flipped, mixed); every case carries its scene"""
    g, p = vc.general(), vc.planar()
    gs, ps = g["scene"], p["scene"]
    c60 = p["claims"][1]                                        # the matches of planar-60%-eight
    rng = np.random.default_rng(5)
    m30, m70 = (vc.make_matches(ps, 2, 3, 300, share, rng) for share in (0.3, 0.7))
    m80 = vc.make_matches(ps, 2, 3, 300, 0.8, np.random.default_rng(PLANAR_80_SEED))
    top = np.random.default_rng(TOP_UP_SEED)                    # the wrong matches that replace those on a used keypoint
    planar_claims = [_case(ps, "planar-30%", 2, 3, *same_share(ps, 2, 3, *m30, top)),
                     _case(ps, "planar-60%", 0, 1, *same_share(ps, 0, 1, c60["matches"], c60["planted"], top)),
                     _case(ps, "planar-70%", 2, 3, *same_share(ps, 2, 3, *m70, top)), _case(ps, "planar-80%", 2, 3, *same_share(ps, 2, 3, *m80, top))]
    c30 = g["claims"][0]                                        # the matches of general-30%
    nan = vc.make_matches(gs, 3, 1, 200, 0.3, np.random.default_rng(GENERAL_NAN_SEED), with_nan=True)
    general_claims = [_case(gs, "general-30%", 0, 1, *same_share(gs, 0, 1, c30["matches"], c30["planted"], top)),
                      _case(gs, "general-30%-nan", 3, 1, *same_share(gs, 3, 1, *nan, top))]
    rng = np.random.default_rng(81)
    sizes = [_case(ps, f"m={m}", *vc.IMAGE_PAIRS[k % len(vc.IMAGE_PAIRS)], *make_distinct(ps, *vc.IMAGE_PAIRS[k % len(vc.IMAGE_PAIRS)], m, 0.3, rng),
                   hypotheses=H_SMALL) for k, m in enumerate(SIZES)]
    m65 = make_distinct(ps, 0, 1, 65, 0.3, rng)
    h_edges = [_case(ps, f"H={H}", 0, 1, *m65, hypotheses=H) for H in H_EDGES]
    same = np.tile(np.array([[5, 5]], np.int32), (40, 1))
    special = [_case(ps, "one-match-repeated", 0, 1, same, np.zeros(40, bool), hypotheses=H_SMALL)]
    col = [_case(collinear_scene(), "three-collinear-in-lo", 0, 1, np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.int32), np.zeros(4, bool),
                 hypotheses=H_SMALL, min_inliers=0)]
    fm, fp = make_distinct(ps, 1, 3, 150, 0.3, rng)
    flipped = [_case(ps, "lo-hi", 1, 3, fm, fp, hypotheses=H_SMALL),
               _case(ps, "hi-lo", 3, 1, np.ascontiguousarray(fm[:, ::-1]), fp, hypotheses=H_SMALL)]
    # the mixed batch on the scene of both: planar and general pairs alternate; every fifth pair holds image 1 of its scene
    # and matches on its keypoints that do not undistort
    bs = both()
    ms = list(SIZES) + [int(x) for x in rng.integers(10, 400, 30)]
    mixed = []
    for k, m in enumerate(ms):
        planar = k % 2 == 0
        sc, off = (ps, PLANAR_OFFSET) if planar else (gs, 0)
        nan = k % 5 == 0
        a, b = ((0, 1), (1, 2), (3, 1))[(k // 5) % 3] if nan else vc.IMAGE_PAIRS[(k + 3) % len(vc.IMAGE_PAIRS)]
        mm, pl = make_distinct(sc, a, b, m, 0.3, rng, with_nan=nan)
        mixed.append(dict(_case(bs, f"mixed-{k}-{'planar' if planar else 'general'}", a + off, b + off, mm, pl, hypotheses=H_SMALL), planar=planar))
    return dict(planar_claims=planar_claims, general_claims=general_claims, sizes=sizes, h_edges=h_edges, special=special, collinear=col,
                flipped=flipped, mixed=mixed)


def options(case, **over):
    return dict(vo.DEFAULTS, intr=case["scene"]["intr"], **dict(case["opts"], **over))


def case_points(case):
    return vo.points(case["scene"]["xy"], case["a"], case["b"], case["matches"])


def _key(case, o):
    return (case["scene"]["rng_seed"], case["name"], case["a"], case["b"], tuple(sorted((k, v) for k, v in o.items() if k != "intr")))


_HYP, _PAIR, _PAIR_E = {}, {}, {}


def oracle_hypotheses(case, **over):
    """(Hm, count, idx, margin) of the case under the homography, computed once and shared"""
    o = options(case, **over)
    key = _key(case, o)
    if key not in _HYP:
        _HYP[key] = ho.hypotheses(case_points(case), min(case["a"], case["b"]), max(case["a"], case["b"]), with_margin=True, **o)
    return _HYP[key]


def oracle_pair(case, **over):
    """the homography run of the case"""
    o = options(case, **over)
    key = _key(case, o)
    if key not in _PAIR:
        _PAIR[key] = ho.verify_pair(case_points(case), min(case["a"], case["b"]), max(case["a"], case["b"]), **o)
    return _PAIR[key]


def oracle_pair_E(case, **over):
    """the essential run of the case (method 0 unless `over` says otherwise)"""
    o = options(case, **over)
    key = _key(case, o)
    if key not in _PAIR_E:
        lo, hi = min(case["a"], case["b"]), max(case["a"], case["b"])
        sc = case["scene"]
        _PAIR_E[key] = vo.verify_pair(case_points(case), lo, hi, vo.relative_rotation(sc["Rcw"][lo], sc["Rcw"][hi]), **o)
    return _PAIR_E[key]


def oracle_auto(case, planar_ratio=ho.PLANAR_RATIO, **over):
    return ho.verify_auto(oracle_pair_E(case, **over), oracle_pair(case, **over), planar_ratio)


def all_cases():
    """every case the GPU tests form hypotheses of"""
    c = cases()
    return c["planar_claims"] + c["general_claims"] + c["sizes"] + c["h_edges"] + c["special"] + c["collinear"] + c["flipped"] + c["mixed"]
