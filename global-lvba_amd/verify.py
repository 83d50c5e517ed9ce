"""Two-view verification of putative matches on the GPU: batched RANSAC over many image pairs at once (lvba_verify_*; the rule is
in include/lvba_hip.h).  Opt-in: nothing imports this module unless verification is asked for."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OPTION_NAMES = L.option_names(L.VerifyOpts)
EIGHT_POINT, KNOWN_ROTATION = 0, 1
OK, TOO_FEW_MATCHES, NO_MODEL, TOO_FEW_INLIERS = 0, 1, 2, 3
STATUS_NAMES = ("ok", "too_few_matches", "no_model", "too_few_inliers")
MODEL_ESSENTIAL, MODEL_HOMOGRAPHY, MODEL_AUTO = 0, 1, 2
MODEL_NAMES = ("essential", "homography", "auto")
PLANAR_RATIO = 0.8


def model_code(model):
    """LVBA_VERIFY_MODEL_* of "essential" | "homography" | "auto" (or of the code itself)"""
    if model in MODEL_NAMES:
        return MODEL_NAMES.index(model)
    if isinstance(model, (int, np.integer)) and not isinstance(model, bool):
        return int(model)                       # an unknown code is the library's to refuse
    raise ValueError(f"unknown verification model {model!r}; one of {MODEL_NAMES}")


def verify_opts(lib=None, **kw):
    """lvba_verify_opts: the defaults (eight-point, 1024 hypotheses, 2 refits, 15 inliers, 4 px, seed 0) with `kw` over them."""
    return L.make_opts(L.VerifyOpts, "verification", **kw)


class Verifier(L.Handle):
    """The undistorted keypoints of a set of images resident on a GPU.  keypoints: a sequence of [n_i, 2] pixel arrays (rounded to
    fp32); intr (fx, fy, cx, cy, k1, k2, p1, p2); Rcw [M, 3, 3] = the rotations of T_cam<-world, or None (then only the pose-free
    eight-point method is available)."""
    _destroy = "lvba_verify_destroy"

    def __init__(self, keypoints, intr, Rcw=None, device=0):
        self.lib = L.load()
        uv, self.off = L.flatten_rows(keypoints, np.float32, 2)
        self.n_images = len(self.off) - 1
        self.counts = np.diff(self.off)
        intr = np.ascontiguousarray(intr, np.float64).reshape(8)
        R = None if Rcw is None else np.ascontiguousarray(Rcw, np.float64).reshape(self.n_images, 9)
        self.has_rotations = R is not None
        self.device = int(device)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_verify_create(self.device, self.n_images, self.off.ctypes.data, uv.ctypes.data, intr.ctypes.data,
                                            R.ctypes.data if R is not None else None, C.byref(self._h)))

    def pairs_csr(self, pairs, matches, match_off, capacity=None, model="essential", planar_ratio=PLANAR_RATIO, **opts):
        """(inliers int32 [n, 2], inlier_off int64 [P + 1], report): the C call as it is.  `capacity` defaults to the number of
        matches, which no result can exceed; inlier_off holds the true offsets also where they pass a smaller capacity.
        model "essential" (the default) is lvba_verify_pairs; "homography" and "auto" go through lvba_verify_pairs_model, and the
        report gains kind (0 essential, 1 homography: what report["E"] of that pair is), n_inliers_E and n_inliers_H (-1 where
        that model was not run).  planar_ratio: the E-or-H choice of "auto"."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
        match_off = np.ascontiguousarray(match_off, np.int64)
        P = len(pairs)
        if len(match_off) != P + 1:
            raise ValueError("match_off must hold one offset per pair and the total")
        o = verify_opts(self.lib, **opts)
        cap = int(len(matches) if capacity is None else capacity)
        inliers = np.zeros((max(cap, 0), 2), np.int32)
        off = np.zeros(P + 1, np.int64)
        E = np.zeros((P, 9))
        status, n_inl, best_h = (np.zeros(P, np.int32) for _ in range(3))
        code = model_code(model)
        extra = {}
        if code == MODEL_ESSENTIAL:
            L.check(self.lib.lvba_verify_pairs(self._h, P, pairs.ctypes.data, match_off.ctypes.data, matches.ctypes.data, C.byref(o), cap,
                                               off.ctypes.data, inliers.ctypes.data, E.ctypes.data, status.ctypes.data, n_inl.ctypes.data,
                                               best_h.ctypes.data))
        else:
            kind, n_E, n_H = (np.zeros(P, np.int32) for _ in range(3))
            L.check(self.lib.lvba_verify_pairs_model(self._h, P, pairs.ctypes.data, match_off.ctypes.data, matches.ctypes.data, C.byref(o), code,
                                                     float(planar_ratio), cap, off.ctypes.data, inliers.ctypes.data, E.ctypes.data,
                                                     kind.ctypes.data, status.ctypes.data, n_inl.ctypes.data, best_h.ctypes.data,
                                                     n_E.ctypes.data, n_H.ctypes.data))
            extra = dict(kind=kind, n_inliers_E=n_E, n_inliers_H=n_H)
        report = dict(E=E.reshape(P, 3, 3), status=status, n_inliers=n_inl, n_matches=np.diff(match_off).astype(np.int64), best_h=best_h, **extra)
        return inliers[:min(int(off[-1]), cap)], off, report

    def pairs(self, pairs, matches, **opts):
        """(inlier_matches, report): one int32 [m, 2] array per pair in the order of `pairs` (empty arrays are kept), and a dict
        of arrays E [P, 3, 3], status, n_inliers, n_matches, best_h; with model="homography" or "auto" (pairs_csr) also kind,
        n_inliers_E and n_inliers_H."""
        flat, off = L.flatten_rows(matches, np.int32, 2)
        inl, ioff, report = self.pairs_csr(pairs, flat, off, **opts)
        return [inl[ioff[p]:ioff[p + 1]] for p in range(len(ioff) - 1)], report

    def hypotheses(self, a, b, matches, model="essential", **opts):
        """(E float64 [H, 3, 3], count int32 [H]): every hypothesis of the pair before the choice, without refinement; an
        invalid one has E = 0 and count = -1.  model="homography": the homographies (lvba_verify_hypotheses_homography)."""
        code = model_code(model)
        if code not in (MODEL_ESSENTIAL, MODEL_HOMOGRAPHY):
            raise ValueError("hypotheses are those of one model: \"essential\" or \"homography\"")
        o = verify_opts(self.lib, **opts)
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
        H = max(int(o.hypotheses), 0)
        E, count = np.zeros((H, 9)), np.zeros(H, np.int32)
        fn = self.lib.lvba_verify_hypotheses if code == MODEL_ESSENTIAL else self.lib.lvba_verify_hypotheses_homography
        L.check(fn(self._h, int(a), int(b), len(m), m.ctypes.data, C.byref(o), E.ctypes.data, count.ctypes.data))
        return E.reshape(H, 3, 3), count

    def score(self, a, b, matches, E, max_error_px=4.0):
        """bool [m]: which matches of the pair (a, b) are inliers of E (lo -> hi)."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
        E = np.ascontiguousarray(E, np.float64).reshape(9)
        mask = np.zeros(len(m), np.uint8)
        L.check(self.lib.lvba_verify_score(self._h, int(a), int(b), len(m), m.ctypes.data, E.ctypes.data, float(max_error_px), mask.ctypes.data))
        return mask.astype(bool)

    def score_homography(self, a, b, matches, Hm, max_error_px=4.0):
        """bool [m]: which matches of the pair (a, b) pass the symmetric transfer test of the homography Hm (lo -> hi)."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
        Hm = np.ascontiguousarray(Hm, np.float64).reshape(9)
        mask = np.zeros(len(m), np.uint8)
        L.check(self.lib.lvba_verify_score_homography(self._h, int(a), int(b), len(m), m.ctypes.data, Hm.ctypes.data, float(max_error_px),
                                                      mask.ctypes.data))
        return mask.astype(bool)


def verify_pairs(keypoints, pairs, matches, intr, Rcw=None, device=0, **opts):
    """Verifier(keypoints, intr, Rcw).pairs(pairs, matches) in one call; `opts` may hold model and planar_ratio."""
    with Verifier(keypoints, intr, Rcw=Rcw, device=device) as v:
        return v.pairs(pairs, matches, **opts)


def summary(pairs, report):
    """The report as plain Python, for a JSON file: per pair the status and the counts, plus the totals.  Where the report
    holds `kind` (model="homography" or "auto") every pair also gets its model and the two models' counts, and the totals the
    number of OK pairs that were taken for a plane."""
    per = [dict(pair=[int(a), int(b)], status=STATUS_NAMES[int(s)], n_matches=int(m), n_inliers=int(n))
           for (a, b), s, m, n in zip(np.asarray(pairs).reshape(-1, 2), report["status"], report["n_matches"], report["n_inliers"])]
    ok = np.asarray(report["status"]) == OK
    out = dict(pairs=per, n_pairs=len(per), n_pairs_ok=int(ok.sum()), n_matches=int(np.sum(report["n_matches"])),
               n_inliers=int(np.asarray(report["n_inliers"])[ok].sum()))
    if "kind" in report:
        for rec, k, ne, nh in zip(per, report["kind"], report["n_inliers_E"], report["n_inliers_H"]):
            rec.update(model=MODEL_NAMES[int(k)], n_inliers_E=int(ne), n_inliers_H=int(nh))
        out["n_pairs_planar"] = int((ok & (np.asarray(report["kind"]) == MODEL_HOMOGRAPHY)).sum())
    return out
