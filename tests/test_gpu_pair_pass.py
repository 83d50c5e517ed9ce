"""The pair pass (balm_pair_col_kernel, balm_pair_staged_kernel, balm_pair_reduce_kernel and the device-built lists of
pair_lists.hip) held to the C oracle block by block AT THE EDGES OF ITS ITEM LISTS: the problems of tests/pair_cases.py, each a few
hundred voxels laid out so that one piece of the kernels' index arithmetic runs (tests/test_pair_cases_host.py shows on the CPU
that every case holds its edge, that no block lies under block_parity's floor and that one dropped or doubled pair moves its
block by far more than the bar).

Per case: lvba_balm_pair_layout must equal the item list predicted from the documented rules (form, cut, window, every item's
length and destination in order, the partial blocks) -- a case that does not reach its edge fails there --; eval(poses_init)
against COracle.eval_sparse at the project's bars (worst block 1e-8, weight outside the listed blocks 1e-12, g and cost 1e-8,
H == H.T bitwise); and the evaluation repeated after one at other poses must give the first one's bits (stale partial blocks,
stale LDS, order-dependent sums).  LVBA_PAIR_WINDOW and LVBA_Y32 are read when a handle is built.

Measured on the MI355X, worst block against the oracle (bar 1e-8): the column kernel 7.3e-14 ... 1.3e-12 over its cases, the
16-lane kernel on the same problems the same to three digits, the two kernels apart by at most 4.6e-16 of a block (printed per
case, not asserted); the 16-lane cases 1.1e-14 ... 5.7e-13; fp32 records 5.3e-8 ... 9.0e-8 (bar 5e-6); the visual stage's worst
camera block 1.2e-14.  A scratch build whose column kernel took its round count from lanes 0..7 only (drops pairs, reads nothing
more) failed the reducer and mixed cases at 6.8e-2 and 3.2e-2 and passed everything else, as the item lists predict.
"""
from collections import Counter

import numpy as np
import pytest

import pair_cases as pc

pytestmark = pytest.mark.gpu

BLOCK_BAR, OUTSIDE_BAR, G_BAR, Y32_BAR = 1e-8, 1e-12, 1e-8, 5e-6
_ORACLE, _RUNS = {}, {}


def _oracle(oracle_mod, name):
    if name not in _ORACLE:
        d = pc.problem(name)
        co = oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"])
        _ORACLE[name] = co.eval_sparse(d["poses_init"])
    return _ORACLE[name]


def _run(pkg, monkeypatch, name, window, y32=False):
    """layout, info and the evaluations at poses_init, poses_gt, poses_init of one handle (kept for the tests that share it)"""
    key = (name, window, y32)
    if key not in _RUNS:
        monkeypatch.setenv("LVBA_PAIR_WINDOW", str(window))
        monkeypatch.setenv("LVBA_Y32", "1" if y32 else "0")
        d = pc.problem(name)
        with pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]) as prob:
            lay, info = prob.pair_layout(), prob.info()
            first = prob.eval(d["poses_init"])
            prob.eval(d["poses_gt"])
            third = prob.eval(d["poses_init"])
        _RUNS[key] = (lay, info, first, third)
    return _RUNS[key]


def _check_layout(lay, info, pred, form=None):
    items = pred["items"]
    assert lay["form"] == (pred["form"] if form is None else form)
    assert (lay["cut"], lay["window_voxels"]) == (pred["cut"], pred["window_voxels"])
    assert lay["item_len"].tolist() == [i.len for i in items]                        # every item, in order
    assert (lay["n_items"], lay["n_multi"], lay["n_partial"]) == (len(items), pred["n_multi"], pred["n_partial"])
    assert (lay["longest_item"], lay["longest_multi"]) == (pred["longest_item"], pred["longest_multi"])
    Bb1 = info["band_blocks"] + 1
    k, want = 0, []
    for i in items:                                   # a block of one item goes straight to its slot, the others to partial
        want.append(-1 - k if i.partial else i.J * Bb1 + (i.I - i.J))                # blocks numbered in item order
        k += i.partial
    assert lay["item_slot"].tolist() == want
    assert Counter((i.I, i.J) for i, s in zip(items, lay["item_slot"]) if s < 0) == pred["partials"]
    assert info["n_blocks"] == len({(i.I, i.J) for i in items}) and info["n_pairs"] == pred["Q"]


def _check_oracle(oracle_mod, name, res, block_bar=BLOCK_BAR):
    H, g, c = res
    bi, bj, blocks, gc, cc = _oracle(oracle_mod, name)
    worst, outside = oracle_mod.block_parity(H, bi, bj, blocks)
    assert worst <= block_bar, (name, worst)
    assert outside <= OUTSIDE_BAR, (name, outside)
    assert np.abs(g - gc).max() <= G_BAR * np.abs(gc).max() and abs(c - cc) <= G_BAR * abs(cc)
    assert np.array_equal(H, H.T)
    return worst


def _check_repeat(first, third):
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2] == third[2]


@pytest.mark.parametrize("name", pc.COL_CASES)
def test_column_kernel_case(pkg, oracle_mod, monkeypatch, name):
    c = pc.CASES[name]
    lay, info, first, third = _run(pkg, monkeypatch, name, c.window)
    _check_layout(lay, info, pc.prediction(name))
    worst = _check_oracle(oracle_mod, name, first)
    _check_repeat(first, third)
    print(f"pair_pass {name} form {lay['form']} items {lay['n_items']} partial {lay['n_partial']}: worst block {worst:.2e}")


@pytest.mark.parametrize("name", pc.COL_CASES)
def test_both_kernels_on_the_same_problem(pkg, oracle_mod, monkeypatch, name):
    """The column cases once more with LVBA_PAIR_WINDOW=0: the 16-lane kernel on the same problem, held to the oracle as well.  The
    worst per-block difference between the two kernels is printed, not asserted: the earliest signal for the next pair-pass change."""
    c = pc.CASES[name]
    lay, info, first, third = _run(pkg, monkeypatch, name, 0)
    _check_layout(lay, info, pc.prediction(name, 0))
    assert lay["form"] == 0
    worst = _check_oracle(oracle_mod, name, first)
    _check_repeat(first, third)
    Hc = _run(pkg, monkeypatch, name, c.window)[2][0]
    bi, bj = _oracle(oracle_mod, name)[:2]
    N = c.N
    lane_blocks = first[0].reshape(N, 6, N, 6)[bi, :, bj, :]
    diff = oracle_mod.block_parity(Hc, bi, bj, lane_blocks)[0]
    print(f"pair_pass {name} 16-lane items {lay['n_items']}: worst block {worst:.2e}; column kernel - 16-lane kernel, worst block {diff:.2e}")


@pytest.mark.parametrize("name", pc.LANE_CASES)
def test_lane_kernel_case(pkg, oracle_mod, monkeypatch, name):
    lay, info, first, third = _run(pkg, monkeypatch, name, 0)
    _check_layout(lay, info, pc.prediction(name))
    assert lay["form"] == 0
    worst = _check_oracle(oracle_mod, name, first)
    _check_repeat(first, third)
    print(f"pair_pass {name} form 0 cut {lay['cut']} items {lay['n_items']} partial {lay['n_partial']}: worst block {worst:.2e}")


@pytest.mark.parametrize("name", pc.Y32_CASES)
def test_fp32_records_case(pkg, oracle_mod, monkeypatch, name):
    """LVBA_Y32=1 at that mode's bars: cost, g and the diagonal blocks are the fp64-record run's bits, the off-diagonal blocks stay
    within 5e-6 of the oracle (block by block)."""
    c = pc.CASES[name]
    lay, info, first, third = _run(pkg, monkeypatch, name, c.window, y32=True)
    assert info["y_fp32"] == 1
    _check_layout(lay, info, pc.prediction(name), form=2)
    H0, g0, c0 = _run(pkg, monkeypatch, name, c.window)[2]
    H1, g1, c1 = first
    assert c1 == c0 and np.array_equal(g1, g0)
    N = c.N
    d0, d1 = H0.reshape(N, 6, N, 6), H1.reshape(N, 6, N, 6)
    for i in range(N):
        assert np.array_equal(d0[i, :, i, :], d1[i, :, i, :])
    assert not np.array_equal(H1, H0)                                                # it did take effect
    worst = _check_oracle(oracle_mod, name, first, block_bar=Y32_BAR)
    _check_repeat(first, third)
    print(f"pair_pass {name} fp32 records: worst block {worst:.2e}")


def test_a_layout_capacity_too_small_is_refused(pkg, monkeypatch):
    import ctypes as C
    monkeypatch.setenv("LVBA_PAIR_WINDOW", "0")
    d = pc.problem("short_array")
    L = pkg._lib
    with pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"]) as prob:
        out, buf = L.PairLayout(), np.full(8, -7, np.int64)
        assert prob.lib.lvba_balm_pair_layout(prob._h, C.byref(out), buf.ctypes.data, None, 2) == L.ERR_ARG
        assert (buf == -7).all() and out.n_items == 6
        assert prob.lib.lvba_balm_pair_layout(prob._h, C.byref(out), buf.ctypes.data, None, 8) == L.OK
        assert buf[:6].sum() == 11 and (buf[6:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the visual stage shares the pass through block_system.hip
# ---------------------------------------------------------------------------------------------------------------------------
VIS_WINDOW = 128


def _visual_problem(synth):
    """300 tracks of four consecutive cameras out of twelve, thinned so that one camera pair is joined by exactly ONE track: with
    windows of 128 landmarks the lists of neighbouring cameras hold more than 32 pairs per window (cut), and that block is a list
    of one pair."""
    d = synth.make_visual_problem(n_cams=12, n_tracks=300, seed=11, track_len=4, invalid_frac=0.0)
    off, cam = d["obs_off"], d["obs_cam"]
    tracks = [tuple(int(c) for c in cam[off[t]:off[t + 1]]) for t in range(len(off) - 1)]
    cnt = Counter((b, a) for tr in tracks for x, a in enumerate(tr) for b in tr[x + 1:])
    lone = min((b for b in cnt if b[1] > 0), key=lambda b: (cnt[b], b))   # not camera 0: its blocks are decoupled
    has = [t for t, tr in enumerate(tracks) if lone[0] in tr and lone[1] in tr]
    keep = np.array([t for t in range(len(tracks)) if t not in has[1:]])
    k = np.diff(off)[keep]
    obs = np.concatenate([np.arange(off[t], off[t + 1]) for t in keep])
    out = dict(d, obs_off=np.concatenate([[0], np.cumsum(k)]).astype(np.int64), obs_cam=cam[obs], obs_uv=d["obs_uv"][obs])
    for f in ("X", "X_gt", "plane", "valid"):
        out[f] = d[f][keep]
    return out, [tracks[t] for t in keep], lone


@pytest.mark.parametrize("radius", [1e4, 3.0])
def test_reduced_camera_system_at_a_cut_list(pkg, synth, monkeypatch, radius):
    """test_reduced_camera_system_matches_oracle of tests/test_gpu_visual.py (its set-up, its bars) on a problem whose camera-pair
    lists are windowed: the column kernel, a list cut at 32 inside one landmark window, and a list of one pair."""
    from oracle import visual_oracle as vo
    monkeypatch.setenv("LVBA_PAIR_WINDOW", str(VIS_WINDOW))
    d, tracks, lone = _visual_problem(synth)
    assert d["valid"].all()
    pred = pc.predict(12, tracks, VIS_WINDOW)
    runs = Counter()
    for i in pred["items"]:
        runs[(i.win, i.I, i.J)] += i.len
    assert pred["form"] == 1 and max(runs.values()) > 32 and sum(i.len for i in pred["items"] if (i.I, i.J) == lone) == 1
    prob = pkg.VisualProblem(12, d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"], d["valid"], d["intr"])
    orc = vo.VisualOracle(vo.VisualProblem(d["q"], d["t"], d["X"], d["obs_off"], d["obs_cam"], d["obs_uv"], d["plane"],
                                           d["valid"], d["intr"]))
    lay, info = prob.pair_layout(), prob.info()
    _check_layout(lay, info, pred)
    assert lay["form"] == 1 and lay["longest_item"] == 32 and lay["n_partial"] > 0 and 1 in lay["item_len"]
    q, t, X = orc.state()
    r, J = orc.residuals_and_jacobian(q, t, X)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    J = J * scale
    D2 = np.clip((J * J).sum(0), 1e-6, 1e32) / radius
    A = J.T @ J + np.diag(D2)
    g = J.T @ r
    nc = orc.n_cam
    B, E, Cm = A[:nc, :nc], A[:nc, nc:], A[nc:, nc:]
    Ci = np.linalg.inv(Cm)
    S_ref = B - E @ Ci @ E.T
    rhs_ref = g[:nc] - E @ (Ci @ g[nc:])
    S, rhs, c = prob.linearize(q, t, X, radius)
    from conftest import rel
    assert abs(c - 0.5 * r @ r) <= 1e-10 * (0.5 * r @ r)
    assert rel(S[6:, 6:], S_ref) <= 1e-9
    assert rel(rhs[6:], rhs_ref) <= 1e-9
    assert np.abs(S[:6, 6:]).max() == 0.0 and np.abs(rhs[:6]).max() == 0.0
    assert np.array_equal(S, S.T)
    # block by block, the one-pair block included
    Sb, Rb = S[6:, 6:].reshape(11, 6, 11, 6), S_ref.reshape(11, 6, 11, 6)
    err = max(np.abs(Sb[i - 1, :, j - 1, :] - Rb[i - 1, :, j - 1, :]).max() / np.abs(Rb[i - 1, :, j - 1, :]).max()
              for i, j in {(i.I, i.J) for i in pred["items"]} if j > 0)
    print(f"pair_pass visual radius {radius:g}: items {lay['n_items']} partial {lay['n_partial']}, worst camera block {err:.2e}, lone block {lone}")
    S2, rhs2, _ = prob.linearize(q, t, X, radius)
    assert np.array_equal(S, S2) and np.array_equal(rhs, rhs2)
