"""The marginal pose covariance (lvba_balm_covariance: csrc/ldlt_selinv.h, driven from ldlt.hip and lvba_api.hip) against a refined
inverse, at the edges of its panel geometry.

What is inverted and what it is compared with.  The system is taken from the handle: H from prob.eval_blocks(x) at the ground-truth
poses x; the covariance call evaluates again at the same x, the evaluation is bit-reproducible, so that H is exactly the matrix the
call factorises and the evaluation's own noise (~1e-9 against the oracle's Hessian) stays out of the comparison.  H is permuted
into the handle's internal pose order (prob.ordering()), where the panel geometry is the kernels', and the anchor applied as
ldlt_anchor_kernel applies it (cov_oracle.anchor_lower).  The reference is cov_oracle.inv of that matrix (LAPACK inverse + two
Newton steps); the yardstick is the fp64 restatement of the kernels' recurrence on the same matrix in the same order
(cov_oracle.selected_inverse), whose factor L also shows, per case, that the tiles and slices the row is named for carry non-zero
data (cov_oracle.live_panels; tests/test_covariance_host.py shows on the CPU that a defect planted there misses the bars).

The error is cov_oracle.worst: over all diagonal blocks |dSigma_i|_F / |Sigma_i|_F, over all pairs of poses that share a voxel
|dSigma_ij|_F / sqrt(|Sigma_ii|_F |Sigma_jj|_F).  The bars (cov_oracle.within_bars) on both figures: at most CAP, and at most K times
the yardstick's figure + 16 eps; K and CAP are derived in tests/cov_oracle.py from the sweep below.

The rows: cov_oracle.EDGE_ROWS (make_problem(N, 40 N, band=band, seed=5); band rows without loop closures, the two large dense rows
with the generator's default ones, so that fill reaches the far slices).  Every row runs with three anchors, given as internal
positions p (caller pose perm[p]): 0, 10 (columns 60 .. 65 straddle the first panel boundary) and N - 1.

The sweep on the MI355X (GPU error and its ratio to the yardstick's, for the diagonal blocks and for the pairs; then the larger of
the yardstick's two figures).  "anchor at p": internal position p:
    row, anchor                            diagonal blocks    pairs              yardstick
    11-3-dense anchor at 0                 8.2e-15  0.17    8.3e-15  0.16    5.0e-14
    11-3-dense anchor at 10                2.3e-14  0.83    2.3e-14  0.83    2.8e-14
    48-2-band anchor at 0                  2.5e-13  0.18    2.5e-13  0.18    1.4e-12
    48-2-band anchor at 10                 2.1e-13  0.20    2.3e-13  0.21    1.1e-12
    48-2-band anchor at 47                 6.5e-13  0.24    6.4e-13  0.24    2.7e-12
    64-12-band anchor at 0                 9.1e-14  0.10    9.5e-14  0.10    9.3e-13
    64-12-band anchor at 10                6.6e-14  0.20    6.8e-14  0.20    3.4e-13
    64-12-band anchor at 63                8.3e-14  0.04    8.4e-14  0.04    2.0e-12
    100-6-band anchor at 0                 4.6e-13  0.19    4.9e-13  0.20    2.5e-12
    100-6-band anchor at 10                4.5e-13  0.15    4.5e-13  0.15    3.1e-12
    100-6-band anchor at 99                6.9e-13  0.38    6.9e-13  0.37    1.9e-12
    300-49-band anchor at 0                3.3e-13  0.13    3.2e-13  0.13    2.5e-12
    300-49-band anchor at 10               2.5e-13  0.23    2.5e-13  0.23    1.1e-12
    300-49-band anchor at 299              5.7e-13  0.24    5.8e-13  0.24    2.4e-12
    360-27-band anchor at 0                6.6e-13  0.30    6.6e-13  0.30    2.2e-12
    360-27-band anchor at 10               5.4e-13  0.19    5.4e-13  0.19    2.9e-12
    360-27-band anchor at 359              7.7e-13  0.57    8.2e-13  0.61    1.4e-12
    360-27-dense anchor at 0               4.5e-13  0.22    4.4e-13  0.21    2.1e-12
    360-27-dense anchor at 10              3.6e-13  0.38    3.6e-13  0.37    9.6e-13
    360-27-dense anchor at 359             4.7e-13  0.26    5.2e-13  0.29    1.8e-12
    300-49-dense anchor at 0               4.6e-13  0.18    4.6e-13  0.18    2.5e-12
    300-49-dense anchor at 10              5.7e-13  0.13    5.7e-13  0.13    4.4e-12
    300-49-dense anchor at 299             5.0e-13  0.11    5.2e-13  0.12    4.4e-12
    100-6-band POSE prior, no anchor       3.1e-12  0.66    3.1e-12  0.66    4.7e-12
    300-49-band pairs at the band limit    2.5e-13  0.23    5.6e-14  0.08    1.1e-12
Largest ratio: 0.83 -> K = 16.  Largest yardstick: 4.73e-12 -> CAP = 64 * 4.73e-12 = 3.0e-10.  (The kernels' products are chains
of fused multiply-adds, the restatement's are BLAS calls: the kernels are the more accurate of the two on every row.)  The 11-pose
row's positions 10 and N - 1 coincide; with the anchor there its only window is the anchor's own rows (_assert_live).
Every figure is printed by the tests (pytest -s).
"""
import numpy as np
import pytest

import cov_oracle as co
import prior_oracle as po
from conftest import make_problem

pytestmark = pytest.mark.gpu

ROWS = {r.id: r for r in co.EDGE_ROWS}
ANCHORS = ("first", "straddle", "last")


def _gt(d):
    return np.ascontiguousarray(d["poses_gt"], np.float64).reshape(-1, 12)


class Case:
    """One row: the handle, its order, the matrix it exports at the ground truth (internal order) and the pairs that share a voxel."""

    def __init__(self, pkg, row, priors=None):
        self.row, N = row, row.N
        self.d = make_problem(N, 40 * N, band=row.band, seed=5, **row.problem)
        self.prob = pkg.BalmProblem(N, self.d["voxel_off"], self.d["pose_idx"], self.d["clusters"], **row.handle)
        if priors is not None:
            self.prob.set_priors([pkg.Prior._make("pose", q["i"], q["j"], q["meas"], q["L"], q["oi"], q["oj"]) for q in priors])
        self.x = _gt(self.d)
        bi, bj, blocks, _, _ = self.prob.eval_blocks(self.x)
        self.info = self.prob.info()
        self.perm = self.prob.ordering().astype(np.int64)         # perm[internal position] = caller pose
        self.iperm = np.empty(N, np.int64)
        self.iperm[self.perm] = np.arange(N)
        off = bi != bj
        self.pairs = np.stack([bi[off], bj[off]], 1)
        H = np.zeros((6 * N, 6 * N))
        for i, j, b in zip(bi, bj, blocks):
            H[6 * i:6 * i + 6, 6 * j:6 * j + 6] = b
            H[6 * j:6 * j + 6, 6 * i:6 * i + 6] = b.T
        self.H = H                                                # caller order
        idx = (6 * self.perm[:, None] + np.arange(6)[None, :]).reshape(-1)
        self.Hint = H[np.ix_(idx, idx)]                           # internal order
        self.bw = row.bw(self.info["band_blocks"])

    def check_form(self):
        i, row = self.info, self.row
        if row.store == "band":
            assert (i["use_band"], i["band_blocks"]) == (1, 2 * row.band), i
            assert co.block_bandwidth(self.Hint) <= i["band_blocks"]
        else:
            assert (i["use_band"], i["band_blocks"]) == (0, row.N - 1), i
        table = co.panel_table(row.n, self.bw)
        assert row.reach(table), ("the row's table no longer reaches what it is there for", table)

    def position(self, which):
        return {"first": 0, "straddle": min(10, self.row.N - 1), "last": self.row.N - 1}[which]

    def reference(self, pos):
        """(S, L, yardstick blocks): the refined inverse of the anchored matrix in internal order with the anchor's rows and columns
        zero, the restatement's factor, and the restatement's (diag, pair blocks) in the caller's order; pos None: no anchor"""
        A = self.Hint if pos is None else co.anchor_lower(self.Hint, 6 * pos)
        S = co.inv(A)
        if pos is not None:
            s = slice(6 * pos, 6 * pos + 6)
            S[s] = 0.0
            S[:, s] = 0.0
        Z, L = co.selected_inverse(A, self.bw)
        return S, L, Z

    def figures(self, S, pairs, diag, blocks, avail):
        """cov_oracle.worst of blocks given in the caller's order against S in internal order"""
        return co.worst(S, diag[self.perm], self.iperm[np.asarray(pairs)], blocks, avail)


@pytest.fixture(scope="module")
def cases(pkg):
    made = {}

    def get(rid):
        if rid not in made:
            made[rid] = Case(pkg, ROWS[rid])
        return made[rid]

    yield get
    for c in made.values():
        c.prob.close()


def _hold(tag, err, yard):
    for name, e, y in (("diag", err[0], yard[0]), ("pairs", err[1], yard[1])):
        print(f"cov_edges {tag} {name}: gpu {e:.3e} yardstick {y:.3e} ratio {e / y:.2f}")
    for name, e, y in (("diag", err[0], yard[0]), ("pairs", err[1], yard[1])):
        assert co.within_bars(e, y), (tag, name, e, y)


def _assert_live(c, L, pos=None):
    """The row's features carry non-zero data in the handle's own order, with this anchor.  One exception, by construction: at
    11 poses the only window is the last pose's elements 4 and 5, so with the anchor at position 10 = N - 1 (both "straddle" and
    "last") those rows of L are the anchor's own zeros.  That row is live with the anchor at 0 only; the other two cases still
    check the anchor kernel's writes at the end of the store."""
    for f in c.row.live:
        live = co.live_panels(L, c.bw, f)
        if c.row.N == 11 and pos == c.row.N - 1:
            assert not live
        else:
            assert live, f"{c.row.id}: no panel in which '{f}' carries non-zero data in the handle's order"


@pytest.mark.parametrize("which", ANCHORS)
@pytest.mark.parametrize("rid", list(ROWS))
def test_anchored_covariance_meets_the_refined_inverse(cases, rid, which):
    c = cases(rid)
    c.check_form()
    pos = c.position(which)
    anchor = int(c.perm[pos])
    S, L, Z = c.reference(pos)
    np.linalg.cholesky(co.anchor_lower(c.Hint, 6 * pos))          # positive definite (raises otherwise)
    _assert_live(c, L, pos)
    diag, pb, av = c.prob.covariance(c.x, anchor=anchor, pairs=c.pairs)
    assert av.all()                                               # every pair that shares a voxel lies in the band
    assert np.isfinite(diag).all() and np.isfinite(pb).all()
    assert np.all(diag[anchor] == 0.0)
    yd, yb = co.blocks_of(Z, c.pairs, anchor, order=c.iperm)
    yard = c.figures(S, c.pairs, yd, yb, av)
    err = c.figures(S, c.pairs, diag, pb, av)
    _hold(f"{rid} anchor at {pos}", err, yard)


def test_gauge_fixed_by_a_prior(pkg, oracle_mod):
    """100/6 band, a POSE prior on one pose and no anchor: the pivot kernel's c0 < 0 path, no anchor kernel.  The system is the
    handle's export with the prior synced; that the export includes the prior is confirmed against prior_oracle.PriorOracle."""
    row = ROWS["100-6-band"]
    d = make_problem(row.N, 40 * row.N, band=row.band, seed=5, **row.problem)
    x = _gt(d)
    k = 37
    L6 = np.diag([40.0, 30.0, 20.0, 6.0, 4.0, 2.0])
    L6[4, 1] = 1.0
    R = x[k, :9].reshape(3, 3) @ po.so3_exp([1e-3, -2e-3, 5e-4])
    priors = [po.make_prior("pose", k, np.r_[R.reshape(9), x[k, 9:] + [0.01, -0.005, 0.02]], L6)]
    c = Case(pkg, row, priors)
    try:
        c.check_form()
        Ho, _, _ = po.PriorOracle(oracle_mod.COracle(row.N, d["voxel_off"], d["pose_idx"], d["clusters"]), priors).eval_dense(x)
        Hn, _, _ = oracle_mod.COracle(row.N, d["voxel_off"], d["pose_idx"], d["clusters"]).eval_dense(x)
        s = slice(6 * k, 6 * k + 6)
        e_with = np.abs(c.H - Ho).max() / np.abs(Ho).max()
        print(f"cov_edges prior: export vs oracle + prior {e_with:.2e}; the prior's block is {np.abs(Ho - Hn)[s, s].max() / np.abs(Ho).max():.2e} of |H|")
        assert e_with <= 1e-8
        assert np.abs(Ho - Hn)[s, s].max() > 1e-4 * np.abs(Ho).max()   # (so 1e-8 could not hold without the prior)
        S, L, Z = c.reference(None)
        np.linalg.cholesky(c.Hint)                                # positive definite with the prior alone (raises otherwise)
        _assert_live(c, L)
        diag, pb, av = c.prob.covariance(c.x, pairs=c.pairs)
        assert av.all() and np.isfinite(diag).all() and np.isfinite(pb).all()
        yd, yb = co.blocks_of(Z, c.pairs, None, order=c.iperm)
        _hold("100-6-band POSE prior, no anchor", c.figures(S, c.pairs, diag, pb, av), c.figures(S, c.pairs, yd, yb, av))
    finally:
        c.prob.close()


def _band_pairs(c):
    """internal positions (I, J): at the band limit, one beyond it, and far, at both ends and in the middle"""
    N, Bb = c.row.N, c.info["band_blocks"]
    at = [(5, 5 + Bb), (N - 1 - Bb, N - 1), (N // 2, N // 2 + Bb), (0, Bb)]
    beyond = [(5, 5 + Bb + 1), (N - 2 - Bb, N - 1), (N // 2, N // 2 + Bb + 1), (0, N - 1)]
    return at, beyond


def test_band_limit(cases):
    """300/49 band: a pair at internal distance band_blocks is available (and meets the bars), one at band_blocks + 1 is not."""
    c = cases("300-49-band")
    c.check_form()
    at, beyond = _band_pairs(c)
    pairs = c.perm[np.array(at + beyond)]
    pos = c.position("straddle")
    anchor = int(c.perm[pos])
    diag, pb, av = c.prob.covariance(c.x, anchor=anchor, pairs=pairs)
    assert list(av) == [True] * len(at) + [False] * len(beyond)
    assert np.isfinite(pb[:len(at)]).all() and np.isnan(pb[len(at):]).all()
    S, _, Z = c.reference(pos)
    yd, yb = co.blocks_of(Z, pairs, anchor, order=c.iperm)
    assert np.isfinite(yb[:len(at)]).all()
    _hold("300-49-band pairs at the band limit", c.figures(S, pairs, diag, pb, av), c.figures(S, pairs, yd, yb, av))


def test_gather_orientation(cases):
    """300/49 band: each pair asked for as (i, j) and as (j, i) -- the blocks are exact transposes, with the same avail."""
    c = cases("300-49-band")
    at, beyond = _band_pairs(c)
    pairs = np.concatenate([c.pairs, c.perm[np.array(at + beyond)]])
    both = np.concatenate([pairs, pairs[:, ::-1]])
    anchor = int(c.perm[c.position("straddle")])
    _, pb, av = c.prob.covariance(c.x, anchor=anchor, pairs=both)
    K = len(pairs)
    assert np.array_equal(av[:K], av[K:]) and av[:K].any() and not av[:K].all()
    assert np.array_equal(pb[:K], pb[K:].transpose(0, 2, 1), equal_nan=True)
    assert np.isnan(pb[:K][~av[:K]]).all() and np.isfinite(pb[:K][av[:K]]).all()


@pytest.mark.parametrize("rid", ["300-49-band", "360-27-dense"])
def test_two_calls_give_the_same_bits(cases, rid):
    """The slices and tiles are summed in index order: nothing depends on which workgroup finishes first."""
    c = cases(rid)
    anchor = int(c.perm[c.position("straddle")])
    a = c.prob.covariance(c.x, anchor=anchor, pairs=c.pairs)
    b = c.prob.covariance(c.x, anchor=anchor, pairs=c.pairs)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
