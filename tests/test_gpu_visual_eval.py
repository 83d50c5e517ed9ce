"""The visual stage's evaluation kernels (csrc/visual_kernels.hip: vis_residual_kernel, the column norms, vis_point_kernel,
vis_cam_kernel in both forms, vis_cam_reduce_kernel, vis_back_kernel, vis_apply_kernel) held to the oracle AT THE EDGES OF THEIR
INDEX ARITHMETIC: the problems of tests/visual_eval_cases.py (tests/test_visual_eval_cases_host.py shows on the CPU that every case
sits on its edge and that one dropped observation moves its camera's block and right-hand side by >= 1e-4, five decades over the
bar), each at S in {rule, 1, 2, 3, 5, 64} slices per camera (LVBA_SLICES) x both forms of the camera kernel (LVBA_VIS_CAM_FORM).

Every run first holds lvba_visual_eval_layout to what the rules and the switches predict -- a case that does not reach its slice
count, form or grid fails there -- then, against a reference formed block by block in np.longdouble from the oracle's Jacobian
(visual_eval_cases.reference): the cost (1e-10), EVERY 6 x 6 block of S against sqrt(max|B_II| max|B_JJ|) and every camera's
right-hand side against its largest |Jc^T r| entry (1e-9, the bar of test_reduced_camera_system_matches_oracle held per block),
S == S^T bitwise, nothing outside the co-visibility pattern, the constant camera decoupled, solve() against the reference camera
step, one LM iteration (cameras, landmarks, the trace row at 1e-7, landmarks without a plane bitwise), a second linearize bitwise
equal to the first, and all (S, form) runs of a case against one another.

Bars that the existing files do not give:
  * solve(): 8 n kappa eps of the largest entry -- the a-priori forward bound of a backward-stable solve of the n = 6 M system,
    kappa the condition number of the reference S over the cameras that have observations;
  * the state after one iteration: q 1e-9, t and X 1e-8, the bars test_reduced_camera_system_at_c3_scale_matches_reference_functors
    holds the cameras to after ITS first iteration;
  * between two (S, form) runs of one case only the order of a camera's sum changes: off-diagonal blocks (built by the pair pass
    from the Y records, which do not depend on the slicing) must be the same bits, diagonal blocks and right-hand sides agree
    within _FORM_SPREAD = ten times the largest spread measured on the MI355X.

The LiDAR stage takes S from the same place (block_system.hip): two small problems at LVBA_SLICES in {1, 2, 3, 64} against the C
oracle at the bars of tests/test_gpu_pair_pass.py, and against S = 1 within _BALM_SPREAD.

Measured on the MI355X (worst block / worst right-hand side, bar 1e-9; both forms the same to three digits): camera_lists
1.8e-14 / 1.6e-13, track_lengths 1.8e-15 / 1.3e-13, order 3.0e-14 / 1.1e-12, the gmax cases 1.6e-15 / 7.6e-14, the landmark counts
<= 2.5e-15 / 1.6e-13; solve() <= 4.5e-9 (bar 7.5e-8, order), trace <= 2.1e-10; spread between the runs of a case <= 6.2e-16; LiDAR
worst block 2.1e-10 (bar 1e-8), <= 4.8e-16 from S = 1.  A scratch build whose vis_cam_kernel ended the last slice at
S * (len / S) -- dropping len % S observations -- failed exactly the runs with a list that S does not divide (every sweep case at
S = 2, 3, 5, 64, the robust and the small-radius runs: 51 tests) and passed the other 49.
"""
import numpy as np
import pytest

import visual_eval_cases as vc
from conftest import make_problem

pytestmark = pytest.mark.gpu

BLOCK_BAR, COST_BAR, TRACE_BAR = 1e-9, 1e-10, 1e-7
RADIUS = 1e4
EPS = float(np.finfo(np.float64).eps)
_FORM_SPREAD = 6.3e-15   # ten times the largest spread measured on the MI355X (6.23e-16 of a right-hand side, 5.55e-16 of a diagonal block)
_BALM_SPREAD = 4.8e-15   # ten times the largest measured (4.76e-16 of a diagonal block at S = 64; the gradient 1.19e-16)
_REF, _RUNS = {}, {}


def _reference(name):
    """the reference of one case, built once: system, step, and the first LM iteration from the start values"""
    if name in _REF:
        return _REF[name]
    d = vc.problem(name)
    R = vc.rows(d)
    ref = vc.reference(R, RADIUS)
    M, cam, lm = R["M"], R["cam"], R["lm"]
    LD = np.longdouble
    cost0 = float(0.5 * ((R["r"].astype(LD) ** 2).sum() + (R["rpl"].astype(LD) ** 2).sum()))
    orc = vc.oracle_of(d)
    q1, t1, X1 = orc.plus(d["q"], d["t"], d["X"], vc.oracle_delta(ref))
    R1 = vc.rows(d, q1, t1, X1)
    cost1 = float(0.5 * ((R1["r"].astype(LD) ** 2).sum() + (R1["rpl"].astype(LD) ** 2).sum()))
    Jc = R["Jc"].astype(LD) * ref["scale_cam"][cam][:, None, :]
    Jp = R["Jp"].astype(LD) * ref["scale_pt"][lm][:, None, :]
    m_obs = np.einsum("oki,oi->ok", Jc, ref["step_cam"][cam]) + np.einsum("oki,oi->ok", Jp, ref["step_pt"][lm])
    m_pl = ((R["Jpl"].astype(LD) * ref["scale_pt"]) * ref["step_pt"]).sum(1)
    model = float(-((m_obs * (R["r"] + m_obs / 2)).sum() + (m_pl * (R["rpl"] + m_pl / 2)).sum()))
    act = R["act"]
    step_norm = float(np.sqrt(((q1[1:] - d["q"][1:]) ** 2).sum() + ((t1[1:] - d["t"][1:]) ** 2).sum() + ((X1[act] - d["X"][act]) ** 2).sum()))
    cg, pg = vc.gradient_parts(d, ref)
    cams = np.bincount(cam, minlength=M)
    idx = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in range(1, M) if cams[c] > 0])
    S64 = ref["S"].astype(np.float64)
    pattern = np.eye(M, dtype=bool)
    for i in act:
        t = list(d["tracks"][i])
        pattern[np.ix_(t, t)] = True
    pattern[0, 1:] = pattern[1:, 0] = False                       # the constant camera is decoupled
    rho = (cost0 - cost1) / model
    assert rho > 1e-3, (name, rho)                                  # the reference's own first step is an accepted one
    _REF[name] = dict(d=d, R=R, ref=ref, cost0=cost0, cost1=cost1, model=model, rho=rho, step_norm=step_norm,
                      gmax=float(max(cg.max(), pg.max(initial=0.0))), q1=q1 / np.linalg.norm(q1, axis=1, keepdims=True), t1=t1, X1=X1,
                      kappa=float(np.linalg.cond(S64[np.ix_(idx, idx)])), pattern=pattern, counts=vc.counts(d),
                      bscale=np.array([float(np.abs(ref["B"][c] + np.diag(ref["D2c"][c])).max()) for c in range(M)]))
    return _REF[name]


def _set(monkeypatch, slices, form):
    for var, v in (("LVBA_SLICES", slices), ("LVBA_VIS_CAM_FORM", form)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))


def _problem(pkg, d):
    return pkg.VisualProblem(d["q"].shape[0], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])


def _block_errors(S, rhs, rf):
    """(worst block of S against sqrt(max|B_II| max|B_JJ|), worst camera of the right-hand side against its largest |Jc^T r|)"""
    ref, M = rf["ref"], rf["R"]["M"]
    dS = np.abs(S.astype(np.longdouble) - ref["S"]).reshape(M, 6, M, 6).max(axis=(1, 3)).astype(np.float64)
    eS = dS / np.sqrt(np.outer(rf["bscale"], rf["bscale"]))
    dr = np.abs(rhs.astype(np.longdouble) - ref["rhs"]).reshape(M, 6).max(1).astype(np.float64)
    jmax = np.abs(ref["jtr"]).max(1).astype(np.float64)
    assert (dr[jmax == 0.0] == 0.0).all()                           # a camera without observations, the constant camera: exactly zero
    er = np.divide(dr, jmax, out=np.zeros(M), where=jmax > 0)
    return eS, er


def _run_case(pkg, monkeypatch, name, slices, form):
    rf = _reference(name)
    d, ref = rf["d"], rf["ref"]
    M = d["q"].shape[0]
    cams, lens, Ta, O = rf["counts"]
    _set(monkeypatch, slices, form)
    prob = _problem(pkg, d)
    try:
        # 1. the layout the launchers use is the one the rules and the switches give
        lay = prob.eval_layout()
        assert lay == vc.predict_layout(M, Ta, O, slices, form), (lay, vc.predict_layout(M, Ta, O, slices, form))
        if name == "order":
            assert prob.info()["band_blocks"] == 3                  # the graph's band, not the caller's: the cameras were re-ordered
        # 2. cost
        S, rhs, c = prob.linearize(d["q"], d["t"], d["X"], RADIUS)
        assert abs(c - rf["cost0"]) <= COST_BAR * rf["cost0"]
        assert abs(prob.cost(d["q"], d["t"], d["X"]) - rf["cost0"]) <= COST_BAR * rf["cost0"]
        # 3. every block, every camera's right-hand side
        eS, er = _block_errors(S, rhs, rf)
        print(f"visual_eval {name} S {lay['slices']} form {lay['unit_form']}: worst block {eS.max():.2e} (diagonal {np.diag(eS).max():.2e}), "
              f"worst right-hand side {er.max():.2e}")
        assert eS.max() <= BLOCK_BAR, (name, slices, form, np.unravel_index(eS.argmax(), eS.shape), eS.max())
        assert er.max() <= BLOCK_BAR, (name, slices, form, int(er.argmax()), er.max())
        # 4. symmetry, pattern, the constant camera
        assert np.array_equal(S, S.T)
        S4 = S.reshape(M, 6, M, 6)
        assert np.abs(S4).max(axis=(1, 3))[~rf["pattern"]].max(initial=0.0) == 0.0
        assert np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0
        # 5. the camera step
        x, _ = prob.solve()
        want = ref["step_cam"].reshape(-1).astype(np.float64)
        e_x = np.abs(x - want).max() / np.abs(want).max()
        bar_x = 8 * 6 * M * rf["kappa"] * EPS
        assert e_x <= bar_x, (name, slices, form, e_x, bar_x)
        # 6. one LM iteration from the same start
        (q1, t1, X1), trace, term, rc = prob.refine(d["q"], d["t"], d["X"], max_iter=1)
        assert rc == 0 and len(trace) == 2 and trace[1]["accepted"] == 1
        e_q, e_t, e_X = np.abs(q1 - rf["q1"]).max(), np.abs(t1 - rf["t1"]).max(), np.abs(X1 - rf["X1"]).max()
        assert e_q <= 1e-9 and e_t <= 1e-8 and e_X <= 1e-8, (name, slices, form, e_q, e_t, e_X)
        dead = d["valid"] == 0
        assert np.array_equal(X1[dead], d["X"][dead]) and np.array_equal(t1[0], d["t"][0])
        row = trace[1]
        got = (trace[0]["cost"], trace[0]["gradient_max_norm"], row["cost"], row["cost_change"], row["rho"], row["step_norm"])
        exp = (rf["cost0"], rf["gmax"], rf["cost1"], rf["cost0"] - rf["cost1"], rf["rho"], rf["step_norm"])
        e_tr = max(abs(a - b) / abs(b) for a, b in zip(got, exp))
        assert e_tr <= TRACE_BAR, (name, slices, form, got, exp)
        print(f"visual_eval {name} S {lay['slices']} form {lay['unit_form']}: solve {e_x:.2e} (bar {bar_x:.2e}), after one iteration "
              f"q {e_q:.2e} t {e_t:.2e} X {e_X:.2e}, trace {e_tr:.2e}")
        # 7. the same bits again (after a solve and a refine on the handle)
        S2, rhs2, c2 = prob.linearize(d["q"], d["t"], d["X"], RADIUS)
        assert np.array_equal(S, S2) and np.array_equal(rhs, rhs2) and c == c2
    finally:
        prob.close()
    return S, rhs, x, (q1, t1, X1)


def _spread(rf, a, b):
    """two runs of one case: (diagonal blocks, right-hand sides) apart, in the scales of the bar; off-diagonal blocks: same bits"""
    M = rf["R"]["M"]
    A, B = a[0].reshape(M, 6, M, 6), b[0].reshape(M, 6, M, 6)
    off = ~np.eye(M, dtype=bool)
    assert np.array_equal(A.transpose(0, 2, 1, 3)[off], B.transpose(0, 2, 1, 3)[off])
    eS, er = _block_errors(b[0], b[1], dict(rf, ref=dict(rf["ref"], S=a[0].astype(np.longdouble), rhs=a[1].astype(np.longdouble))))
    return float(eS.max()), float(er.max())


@pytest.mark.parametrize("form", vc.FORMS)
@pytest.mark.parametrize("slices", vc.SLICES)
@pytest.mark.parametrize("name", vc.SWEEP_CASES)
def test_case_at_every_slice_count_and_form(pkg, monkeypatch, name, slices, form):
    if (name, None, None) not in _RUNS:
        _RUNS[(name, None, None)] = _run_case(pkg, monkeypatch, name, None, None)      # neither switch set: today's path
    run = _RUNS[(name, slices, form)] = _run_case(pkg, monkeypatch, name, slices, form)
    # 8. against the run with neither switch set
    sS, sr = _spread(_reference(name), _RUNS[(name, None, None)], run)
    print(f"visual_eval {name} S {slices} form {form}: apart from the default run by {sS:.2e} (diagonal blocks), {sr:.2e} (right-hand side)")
    assert sS <= _FORM_SPREAD and sr <= _FORM_SPREAD, (name, slices, form, sS, sr)


@pytest.mark.parametrize("name", vc.LANDMARK_CASES)
def test_landmark_count_case(pkg, monkeypatch, name):
    _run_case(pkg, monkeypatch, name, None, None)


@pytest.mark.parametrize("radius", [3.0])
def test_camera_lists_at_a_small_radius(pkg, monkeypatch, radius):
    """the LM diagonal at the radius of test_reduced_camera_system_matches_oracle's second row, S = 5 in both forms"""
    rf = _reference("camera_lists")
    d = rf["d"]
    ref = vc.reference(rf["R"], radius, solve=False)
    bscale = np.array([float(np.abs(ref["B"][c] + np.diag(ref["D2c"][c])).max()) for c in range(rf["R"]["M"])])
    for form in vc.FORMS:
        _set(monkeypatch, 5, form)
        prob = _problem(pkg, d)
        try:
            assert (prob.eval_layout()["slices"], prob.eval_layout()["unit_form"]) == (5, form)
            S, rhs, _ = prob.linearize(d["q"], d["t"], d["X"], radius)
        finally:
            prob.close()
        eS, er = _block_errors(S, rhs, dict(rf, ref=ref, bscale=bscale))
        assert eS.max() <= BLOCK_BAR and er.max() <= BLOCK_BAR, (form, eS.max(), er.max())


_ROBUST = {}


@pytest.mark.parametrize("form", vc.FORMS)
def test_robust_kernels_on_the_camera_lists(pkg, monkeypatch, form):
    """the ROBUST instantiations (separate kernels) at S = 3 in both forms, against tests/robust_visual_oracle.py at the bars of
    tests/test_gpu_visual_loss.py (cost 1e-10, S and right-hand side 1e-9 of their largest entry)"""
    import robust_visual_oracle as rvo
    from conftest import rel
    rf = _reference("camera_lists")
    d = rf["d"]
    losses = (("huber", 1.0), ("cauchy", 2.0))
    if not _ROBUST:
        orc = rvo.RobustVisualOracle(vc.oracle_of(d).p, *losses)
        rt, Jt, s, rho0 = orc.correct(*vc.dense(rf["R"]))
        assert (s[orc.block_family == 0] > 1.0).mean() > 0.2 and (rho0 < s).any()    # the losses are engaged
        _ROBUST["ref"] = orc.reduced_system(rt, Jt, s, rho0, RADIUS)
    S_ref, rhs_ref, c_ref = _ROBUST["ref"]
    cams, lens, Ta, O = rf["counts"]
    _set(monkeypatch, 3, form)
    prob = _problem(pkg, d)
    try:
        prob.set_loss(*losses)
        assert prob.eval_layout() == vc.predict_layout(13, Ta, O, 3, form)
        S, rhs, c = prob.linearize(d["q"], d["t"], d["X"], RADIUS)
        S2, rhs2, _ = prob.linearize(d["q"], d["t"], d["X"], RADIUS)
    finally:
        prob.close()
    assert abs(c - c_ref) <= COST_BAR * c_ref
    print(f"visual_eval robust camera_lists S 3 form {form}: S {rel(S[6:, 6:], S_ref):.2e} rhs {rel(rhs[6:], rhs_ref):.2e}")
    assert rel(S[6:, 6:], S_ref) <= 1e-9 and rel(rhs[6:], rhs_ref) <= 1e-9
    assert np.array_equal(S, S.T) and np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0
    assert np.array_equal(S, S2) and np.array_equal(rhs, rhs2)
    _ROBUST[form] = (S, rhs)
    if len(_ROBUST) == 3:
        print(f"visual_eval robust camera_lists: the two forms apart by {rel(_ROBUST[0][0], _ROBUST[1][0]):.2e} (S), "
              f"{rel(_ROBUST[0][1], _ROBUST[1][1]):.2e} (right-hand side)")
        assert rel(_ROBUST[0][0], _ROBUST[1][0]) <= _FORM_SPREAD and rel(_ROBUST[0][1], _ROBUST[1][1]) <= _FORM_SPREAD


@pytest.mark.parametrize("var,value", [("LVBA_SLICES", "0"), ("LVBA_SLICES", "65"), ("LVBA_SLICES", "two"), ("LVBA_SLICES", ""),
                                       ("LVBA_SLICES", "3x"), ("LVBA_VIS_CAM_FORM", "2"), ("LVBA_VIS_CAM_FORM", "-1")])
def test_a_switch_out_of_range_is_refused(pkg, monkeypatch, var, value):
    d = vc.problem("landmarks_17")
    _set(monkeypatch, None, None)
    monkeypatch.setenv(var, value)
    prob = _problem(pkg, d)
    try:
        with pytest.raises(pkg._lib.LvbaError) as e:
            prob.eval_layout()
        assert e.value.code == pkg._lib.ERR_ARG and var in str(e.value)
        with pytest.raises(pkg._lib.LvbaError):
            prob.cost(d["q"], d["t"], d["X"])
        monkeypatch.delenv(var)                                     # the handle was left as it was: it finalises once the value is gone
        assert prob.eval_layout()["slices"] == 1
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the LiDAR stage: the same S
# ---------------------------------------------------------------------------------------------------------------------------
_BALM = {}


def _balm_problem(extra_pose):
    d = make_problem(12, 60, band=4, seed=1)
    if not extra_pose:
        return d
    return dict(d, n_poses=13, poses_init=np.concatenate([d["poses_init"], d["poses_init"][-1:]]))  # a pose no voxel sees


@pytest.mark.parametrize("slices", [1, 2, 3, 64])
@pytest.mark.parametrize("extra_pose", [False, True])
def test_lidar_factor_pass_at_every_slice_count(pkg, oracle_mod, monkeypatch, extra_pose, slices):
    d = _balm_problem(extra_pose)
    N = d["n_poses"]
    if ("oracle", extra_pose) not in _BALM:
        co = oracle_mod.COracle(N, d["voxel_off"], d["pose_idx"], d["clusters"])
        _BALM[("oracle", extra_pose)] = co.eval_sparse(d["poses_init"])
    bi, bj, blocks, gc, cc = _BALM[("oracle", extra_pose)]
    assert vc.rule_slices(N, len(d["pose_idx"])) == 1               # the rule alone never slices this problem
    for s in sorted({1, slices}):
        if (extra_pose, s) in _BALM:
            continue
        _set(monkeypatch, s, None)
        with pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"]) as prob:
            lay, info = prob.eval_layout(), prob.info()
            assert lay == dict(slices=s, unit_form=0, units=N * s, unit_grid=N * s, point_groups=0, back_groups=0, point_grid=0,
                               back_grid=0, n_groups=len(d["voxel_off"]) - 1, n_factors=len(d["pose_idx"]), n_chunks=info["n_chunks"])
            first = prob.eval(d["poses_init"])
            prob.eval(d["poses_gt"] if not extra_pose else np.concatenate([d["poses_gt"], d["poses_gt"][-1:]]))
            third = prob.eval(d["poses_init"])
        assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2] == third[2]
        _BALM[(extra_pose, s)] = first
    H, g, c = _BALM[(extra_pose, slices)]
    worst, outside = oracle_mod.block_parity(H, bi, bj, blocks)
    assert worst <= 1e-8 and outside <= 1e-12, (worst, outside)
    assert np.abs(g - gc).max() <= 1e-8 * np.abs(gc).max() and abs(c - cc) <= 1e-8 * abs(cc)
    assert np.array_equal(H, H.T)
    if extra_pose:
        assert np.abs(H[72:, :]).max() == 0.0 and np.abs(g[72:]).max() == 0.0
    H1, g1, c1 = _BALM[(extra_pose, 1)]
    A, B = H.reshape(N, 6, N, 6), H1.reshape(N, 6, N, 6)
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal(A.transpose(0, 2, 1, 3)[off], B.transpose(0, 2, 1, 3)[off]) and c == c1
    dscale = np.array([max(np.abs(B[i, :, i, :]).max(), 1e-300) for i in range(N)])
    sH = max(np.abs(A[i, :, i, :] - B[i, :, i, :]).max() / dscale[i] for i in range(N))
    sg = np.abs(g - g1).max() / np.abs(g1).max()
    print(f"visual_eval lidar {'13 poses' if extra_pose else '12 poses'} S {slices}: worst block {worst:.2e}; apart from S = 1 by {sH:.2e} "
          f"(diagonal blocks), {sg:.2e} (gradient)")
    assert sH <= _BALM_SPREAD and sg <= _BALM_SPREAD, (sH, sg)
