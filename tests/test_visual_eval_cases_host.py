"""CPU conditions on the problems of tests/visual_eval_cases.py, from the arrays and the oracle alone -- so that
tests/test_gpu_visual_eval.py cannot pass vacuously: every case sits on the edge it is named for (per-camera counts, track
lengths, Ta, O, the slice lengths every S of the sweep gives, the place of the largest gradient entry, a natural camera order
wider than the graph's band); the batched rows and the block-by-block reference are the oracle's own numbers; no diagonal block
lies under the scale floor of the GPU test; and every observation matters -- leaving any single one out moves its camera's
diagonal block and its camera's right-hand side by at least 1000 x the GPU bar of 1e-9, so a dropped or doubled observation
cannot hide under the bar."""
import numpy as np
import pytest

import visual_eval_cases as vc

GPU_BAR = 1e-9
SENSITIVITY = 1000 * GPU_BAR
RADIUS = 1e4


def test_camera_lists_case_holds_every_count():
    d = vc.problem("camera_lists")
    cams, lens, Ta, O = vc.counts(d)
    assert cams.tolist() == vc.CAM_COUNTS == [64, 0, 1, 2, 63, 65, 127, 128, 129, 255, 256, 257, 513]
    assert cams[0] > 0 and Ta == 513 and O == sum(vc.CAM_COUNTS) and d["valid"].all()
    assert vc.rule_slices(13, O) == 1                              # the rule alone never slices this problem
    # what the sweep reaches on these lists: shorter than, equal to and one more than S; empty slices; units no multiple of four
    reach = {(n, S): vc.slice_lengths(n, S) for n in vc.CAM_COUNTS for S in (2, 3, 5, 64)}
    assert reach[(1, 2)] == [0, 1] and reach[(2, 2)] == [1, 1] and reach[(2, 3)] == [0, 1, 1] and reach[(2, 5)] == [0, 0, 1, 0, 1]
    assert reach[(63, 64)].count(0) == 1 and set(reach[(64, 64)]) == {1} and sorted(set(reach[(65, 64)])) == [1, 2]
    assert reach[(0, 64)] == [0] * 64 and sum(reach[(513, 64)]) == 513 and sorted(set(reach[(513, 64)])) == [8, 9]
    assert all(sum(v) == n for (n, S), v in reach.items())
    assert [13 * S % 4 for S in (1, 2, 3, 5, 64)] == [1, 2, 3, 1, 0]  # the wavefront form's early return runs for S = 1, 2, 3, 5
    # the per-lane strides of the two forms (64, 256) are crossed by whole lists at S = 1 and by slices at S = 2
    assert {63, 64, 65, 255, 256, 257} <= set(vc.CAM_COUNTS) and reach[(513, 2)] == [256, 257] and reach[(129, 2)] == [64, 65]


def test_track_lengths_case_holds_every_length():
    d = vc.problem("track_lengths")
    cams, lens, Ta, O = vc.counts(d)
    assert set(vc.TRACK_LENGTHS) | {13} == set(lens.tolist())
    assert {n % 4 for n in lens.tolist()} == {0, 1, 2, 3}          # every count of idle lanes in a quad
    act = np.nonzero(d["valid"])[0]
    tracks = d["tracks"]
    assert any(tracks[i] == tuple(range(13)) for i in act) and any(tracks[i] == (0,) for i in act)
    T = len(tracks)
    dead = np.nonzero(d["valid"] == 0)[0].tolist()
    assert dead[0] == 0 and dead[-1] == T - 1 and 0 < dead[1] < T - 1 and len(dead) == 3
    assert all(len(tracks[i]) > 0 for i in dead)                   # their observations go with them
    assert (act != np.arange(Ta)).all()                            # the compaction moves every index
    assert Ta % 64 not in (0,) and cams.min() >= 3 and O == int(lens.sum())


@pytest.mark.parametrize("Ta", vc.LANDMARK_COUNTS)
def test_landmark_count_cases(Ta):
    d = vc.problem(f"landmarks_{Ta}")
    cams, lens, n, O = vc.counts(d)
    assert n == Ta and d["q"].shape[0] == 4 and cams.min() >= 1
    lay = vc.predict_layout(4, Ta, O)
    assert (lay["slices"], lay["unit_form"], lay["unit_grid"]) == (1, 1, 1)
    # groups of 64 landmarks (point kernel: four per workgroup, back-substitution: one) and blocks of 256 threads
    assert lay["back_grid"] == {1: 1, 15: 1, 16: 1, 17: 1, 63: 1, 64: 1, 65: 2, 255: 4, 256: 4, 257: 5}[Ta]
    assert lay["point_grid"] == {257: 2}.get(Ta, 1)
    blocks = lambda n: max(1, -(-n // 256))
    want = {1: (1, 1, 1), 15: (1, 1, 1), 16: (1, 1, 1), 17: (1, 1, 1), 63: (1, 1, 1), 64: (1, 1, 1), 65: (1, 2, 1),
            255: (3, 4, 2), 256: (3, 4, 2), 257: (4, 5, 2)}[Ta]
    assert (blocks(O), blocks(O + Ta), blocks(4 + Ta)) == want      # vis_residual_kernel's two ranges, vis_apply_kernel


def test_landmark_count_cases_cross_256():
    """O, O + Ta and M + Ta each lie on both sides of a multiple of 256 within the set"""
    o = {Ta: vc.counts(vc.problem(f"landmarks_{Ta}"))[3] for Ta in vc.LANDMARK_COUNTS}
    assert o[64] < 256 < o[65] + 65 and o[255] + 255 <= 1024 < o[257] + 257 and o[255] < 768 < o[257]
    assert 4 + 64 < 256 < 4 + 255 and 4 + 255 > 256


@pytest.mark.parametrize("name,where", [("gmax_landmark", ("lm", vc.GMAX_TA - 1)), ("gmax_last_camera", ("cam", 5)),
                                        ("gmax_neighbour", ("cam", 1))])
def test_gradient_maximum_cases(name, where):
    d = vc.problem(name)
    ref = vc.reference(vc.rows(d), RADIUS, dtype=np.float64, solve=False)
    cg, pg = vc.gradient_parts(d, ref)
    assert vc.GMAX_TA % 64 != 0 and len(pg) == vc.GMAX_TA           # the last landmark sits in a partial group
    kind, at = where
    mine = (pg if kind == "lm" else cg)[at]
    rest = max(np.delete(pg, at).max() if kind == "lm" else pg.max(), np.delete(cg, at).max() if kind == "cam" else cg.max())
    assert mine >= 2.0 * rest, (mine, rest)                         # it IS the maximum, by a clear margin
    orc = vc.oracle_of(d)
    r, J = vc.dense(vc.rows(d))
    assert abs(orc.gradient_max_norm(d["q"], J.T @ r) - mine) <= 1e-12 * mine


def test_order_case_has_a_wider_natural_band():
    d = vc.problem("order")
    M = d["q"].shape[0]
    assert 6 * M > 1024                                             # an ordering is computed from this size on
    nat = max(max(t) - min(t) for t in d["tracks"])
    lab = vc.order_labels()
    pos = np.argsort(lab)
    graph = max(max(pos[list(t)]) - min(pos[list(t)]) for t in d["tracks"])
    assert graph == 3 and nat > 100                                 # the ordering is adopted when it is narrower than the natural one
    assert 20 < pos[0] < M - 20                                     # the constant camera sits inside the band, not at an end


@pytest.mark.parametrize("name", ["landmarks_17", "track_lengths"])
def test_batched_rows_are_the_oracles_rows(name):
    d = vc.problem(name)
    orc = vc.oracle_of(d)
    r0, J0 = orc.residuals_and_jacobian(*orc.state())
    r1, J1 = vc.dense(vc.rows(d))
    assert r0.shape == r1.shape and J0.shape == J1.shape
    assert np.abs(r1 - r0).max() <= 1e-13 * np.abs(r0).max()
    assert np.abs(J1 - J0).max() <= 1e-12 * np.abs(J0).max()
    assert np.array_equal(J1 != 0, J0 != 0)


@pytest.mark.parametrize("name", ["landmarks_65", "track_lengths", "gmax_neighbour"])
def test_block_reference_is_the_dense_schur_complement(name):
    """reference() against VisualOracle's dense fp64 formulas (test_reduced_camera_system_matches_oracle, solve_schur)"""
    d = vc.problem(name)
    orc = vc.oracle_of(d)
    R = vc.rows(d)
    r, J = vc.dense(R)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    D2 = np.clip((Js * Js).sum(0), 1e-6, 1e32) / RADIUS
    A = Js.T @ Js + np.diag(D2)
    g = Js.T @ r
    nc = orc.n_cam
    Ci = np.linalg.inv(A[nc:, nc:])
    S0, rhs0 = A[:nc, :nc] - A[:nc, nc:] @ Ci @ A[nc:, :nc], g[:nc] - A[:nc, nc:] @ (Ci @ g[nc:])
    x0 = orc.solve_schur(Js, r, np.sqrt(D2))
    ref = vc.reference(R, RADIUS)
    S1, rhs1 = ref["S"].astype(np.float64), ref["rhs"].astype(np.float64)
    assert np.abs(S1[6:, 6:] - S0).max() <= 1e-11 * np.abs(S0).max() and np.abs(rhs1[6:] - rhs0).max() <= 1e-11 * np.abs(rhs0).max()
    assert np.abs(S1[:6, 6:]).max() == 0.0 and np.abs(rhs1[:6]).max() == 0.0
    x1 = -np.concatenate([ref["step_cam"][1:].reshape(-1), ref["step_pt"].reshape(-1)]).astype(np.float64)
    kappa = np.linalg.cond(A)
    assert np.abs(x1 - x0).max() <= 64 * kappa * np.finfo(np.float64).eps * np.abs(x0).max()
    assert np.abs(vc.oracle_delta(ref) + x0 * scale).max() <= 64 * kappa * np.finfo(np.float64).eps * np.abs(x0 * scale).max()


@pytest.mark.parametrize("name", vc.NAMES)
def test_no_block_under_the_floor_and_every_observation_matters(name):
    d = vc.problem(name)
    R = vc.rows(d)
    ref = vc.reference(R, RADIUS, dtype=np.float64, solve=False)
    M = R["M"]
    scale = np.array([np.abs(ref["B"][c] + np.diag(ref["D2c"][c])).max() for c in range(M)])
    assert scale.min() >= vc.MIN_DIAG / RADIUS * (1 - 1e-15)        # the LM diagonal keeps every block's scale off zero
    cams = np.bincount(R["cam"], minlength=M)
    worst_S, worst_r, at = np.inf, np.inf, None
    for c in range(1, M):                                           # (camera 0 is constant: zero Jacobian columns)
        if cams[c] == 0:
            continue
        dS, dr, S0, rhs0 = vc.leave_one_out(R, RADIUS, c)
        assert np.abs(S0 - ref["S"][6 * c:6 * c + 6, 6 * c:6 * c + 6]).max() <= 1e-12 * np.abs(S0).max()
        assert np.abs(rhs0 - ref["rhs"][6 * c:6 * c + 6]).max() <= 1e-11 * np.abs(ref["jtr"][c]).max()
        if dS.min() < worst_S:
            worst_S, at = dS.min(), (c, int(cams[c]))
        worst_r = min(worst_r, dr.min())
        assert dS.min() >= SENSITIVITY and dr.min() >= SENSITIVITY, (name, c, int(cams[c]), dS.min(), dr.min())
    print(f"{name}: one observation moves its camera's block by >= {worst_S:.2e} (camera, list {at}), its right-hand side by >= {worst_r:.2e}")
