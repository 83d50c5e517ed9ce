"""CPU tests of the marginal pose covariance (lvba_balm_covariance): the panel recurrence the kernels of csrc/ldlt_selinv.h follow,
restated in numpy on band storage (tests/cov_oracle.py), against a dense inverse; and the C-ABI surface without a device."""
import ctypes as C

import numpy as np
import pytest

import cov_oracle as co
from conftest import make_problem


def _spd_band(n, bw, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for o in range(1, min(bw, n - 1) + 1):
        v = rng.normal(size=n - o)
        A[np.arange(o, n), np.arange(n - o)] = v
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + rng.uniform(0.5, 2.0, size=n)   # diagonally dominant: SPD
    return A


def _check(A, bw, tol=1e-12):
    Z = co.band_inverse(A, bw)
    ref = co.inv(A)
    m = ~np.isnan(Z)
    n = A.shape[0]
    i, j = np.indices((n, n))
    assert np.array_equal(m, np.abs(i - j) <= bw)
    err = np.abs(Z[m] - ref[m]).max() / np.abs(ref).max()
    assert err <= tol, err
    return err


@pytest.mark.parametrize("n,bw,seed", [(200, 30, 0), (331, 70, 1), (150, 100, 2), (64 * 3 + 5, 64, 3)])
def test_recurrence_on_random_spd_bands(n, bw, seed):
    _check(_spd_band(n, bw, seed), bw)


@pytest.mark.parametrize("n", [6, 37, 63])
def test_recurrence_single_partial_panel(n):
    _check(_spd_band(n, n - 1, n), n - 1)


def test_recurrence_dense_case():
    n = 140
    _check(_spd_band(n, n - 1, 7), n - 1)        # bw = n - 1: every entry, the dense store
    _check(_spd_band(n, n - 3, 8), n - 3)        # bw close to n


def test_recurrence_on_an_oracle_hessian_with_an_anchor(oracle_mod):
    d = make_problem(24, 1500, band=4, seed=5)
    orc = oracle_mod.COracle(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"])
    x = orc.damping_iter(d["poses_init"], max_iter=20)[0]
    H, _, _ = orc.eval_dense(x)
    bw = 6 * co.block_bandwidth(H) + 5
    for anchor in (0, 11, 23):
        A = co.anchored(H, anchor)
        Z = co.band_inverse(A, bw)
        ref = co.anchored_inverse(H, anchor)
        keep = np.ones(H.shape[0], bool)
        keep[6 * anchor:6 * anchor + 6] = False
        m = ~np.isnan(Z) & keep[:, None] & keep[None, :]
        err = np.abs(Z[m] - ref[m]).max() / np.abs(ref).max()
        assert err <= 1e-12, (anchor, err)
        s = slice(6 * anchor, 6 * anchor + 6)
        assert np.array_equal(Z[s, s], np.eye(6))   # the identity block of the anchor, coupled to nothing
        assert np.all(Z[s][:, keep][~np.isnan(Z[s][:, keep])] == 0.0)


def test_abi_exports_and_defaults(pkg):
    lib = pkg._lib.load()
    for name in ("lvba_balm_covariance", "lvba_cov_default_opts"):
        assert hasattr(lib, name)
    o = pkg._lib.CovOpts()
    o.anchor, o.min_pivot_ratio = 5, 0.0
    lib.lvba_cov_default_opts(C.byref(o))
    assert o.anchor == -1 and o.min_pivot_ratio == 1e-10
    x = np.zeros(12)
    assert lib.lvba_balm_covariance(None, x, C.byref(o), None, 0, None, None, None, None) == pkg._lib.ERR_ARG


# ---- the dense-array restatement (cov_oracle.selected_inverse) and the rows of tests/test_gpu_covariance_edges.py -----------------
@pytest.mark.parametrize("n,bw,seed", [(200, 30, 0), (331, 70, 1), (150, 100, 2), (64 * 3 + 5, 64, 3), (37, 36, 37), (140, 139, 7),
                                       (140, 137, 8)])
def test_dense_form_agrees_with_the_band_form(n, bw, seed):
    A = _spd_band(n, bw, seed)
    old = co.band_inverse(A, bw)
    new, L = co.selected_inverse(A, bw)
    assert np.array_equal(np.isnan(old), np.isnan(new))
    m = ~np.isnan(old)
    assert np.abs(new[m] - old[m]).max() <= 1e-13 * np.abs(old[m]).max()
    abL, _, _ = co.ldlt_band(co.band_store(A, bw), bw)
    for k, nbe, w0, rend, *_ in co.panel_table(n, bw):
        if rend > w0:
            ref = co._get(abL, w0, rend, k, k + nbe)
            assert np.abs(L[w0:rend, k:k + nbe] - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1.0)


def test_panel_table_geometry():
    for n, bw in ((66, 65), (288, 29), (1800, 593), (2160, 2159)):
        for k, nbe, w0, rend, nw, T, KS, ksz in co.panel_table(n, bw):
            assert w0 == k + nbe and rend == min(w0 + bw, n) and nw == rend - w0 and T == -(-nw // 64)
            if T:
                assert 1 <= KS <= min(co.KSMAX, max(1, 256 // T)) and ksz % 64 == 0
                assert (KS - 1) * ksz < nw <= KS * ksz                     # the slices cover the window, none is empty


def _edge_system(oracle_mod, row):
    """H of the row's problem at the ground-truth poses, natural pose order, and the pairs of poses that share a voxel"""
    d = make_problem(row.N, 40 * row.N, band=row.band, seed=5, **row.problem)
    orc = oracle_mod.COracle(row.N, d["voxel_off"], d["pose_idx"], d["clusters"])
    H, _, _ = orc.eval_dense(np.ascontiguousarray(d["poses_gt"], np.float64).reshape(-1, 12))
    B = np.abs(H).reshape(row.N, 6, row.N, 6).max(axis=(1, 3)) > 0
    bi, bj = np.nonzero(np.tril(B, -1))
    return H, np.stack([bi, bj], 1)


def _figures(S, Zl, bw, pairs, anchor):
    diag, blk = co.blocks_of(co.sym_band(Zl, bw), pairs, anchor)
    return co.worst(S, diag, pairs, blk, np.ones(len(pairs), bool))


@pytest.mark.parametrize("row", co.EDGE_ROWS, ids=lambda r: r.id)
def test_edge_rows_are_live_and_the_bars_bite(oracle_mod, row):
    """Per row, with anchor pose 0: the reach predicate, liveness of every feature the row is named for, the clean restatement
    within the bars against cov_oracle.inv (its yardstick is itself, so this is CAP), and every stage-0 defect, planted in the first
    and the middle panel in which its feature is live, outside the bars in BOTH figures' sense: the diagonal blocks or the pairs
    miss them, and the pairs always do.  anchor_row_kept changes nothing at pose 0 (nothing lies left of the first block), so it is
    planted with the anchors 10 and N - 1."""
    H, pairs = _edge_system(oracle_mod, row)
    bw = row.bw(co.block_bandwidth(H))
    if row.store == "band":
        assert co.block_bandwidth(H) == 2 * row.band
    table = co.panel_table(row.n, bw)
    assert row.reach(table), table
    A = co.anchor_lower(H, 0)
    assert np.linalg.eigvalsh(A).min() > 0
    L, Gs, d = co.ldlt_dense(A, bw)
    for f in row.live:
        assert co.live_panels(L, bw, f), f"{row.id}: no panel in which '{f}' carries non-zero data"
    S = co.inv(A)
    S[:6] = 0.0
    S[:, :6] = 0.0
    clean = co.selinv_dense(L, Gs, d, bw)
    yard = _figures(S, clean, bw, pairs, 0)
    print(f"{row.id}: bw {bw}, yardstick diag {yard[0]:.2e} pairs {yard[1]:.2e}")
    assert co.within_bars(yard[0], yard[0]) and co.within_bars(yard[1], yard[1])
    sites = co.plant_sites(L, bw)
    want = {"tile": "drop_last_tile", "slice": "drop_last_slice", "mid": "drop_mid_slice"}
    for f in row.live:
        assert sites[want[f]]
    assert sites["fp32_x"]
    for kind, where in sites.items():
        for st in where:
            e = _figures(S, co.selinv_dense(L, Gs, d, bw, defect=(st, kind), resume=clean), bw, pairs, 0)
            print(f"{row.id}: {kind} in panel {st}: diag {e[0]:.2e} pairs {e[1]:.2e}")
            assert not co.within_bars(e[0], yard[0]), (kind, st, e, yard)
            assert not co.within_bars(e[1], yard[1]), (kind, st, e, yard)
    for anchor in sorted({min(10, row.N - 1), row.N - 1}):
        A = co.anchor_lower(H, 6 * anchor)
        S = co.inv(A)
        s = slice(6 * anchor, 6 * anchor + 6)
        S[s] = 0.0
        S[:, s] = 0.0
        out = []
        for kept in (False, True):
            Z, _ = co.selected_inverse(co.anchor_lower(H, 6 * anchor, row_kept=kept), bw)
            diag, blk = co.blocks_of(Z, pairs, anchor)
            out.append(co.worst(S, diag, pairs, blk, np.ones(len(pairs), bool)))
        print(f"{row.id}: anchor {anchor}: clean diag {out[0][0]:.2e} pairs {out[0][1]:.2e}; anchor_row_kept diag {out[1][0]:.2e} "
              f"pairs {out[1][1]:.2e}")
        for k in (0, 1):
            assert co.within_bars(out[0][k], out[0][k])
            assert not co.within_bars(out[1][k], out[0][k])


def test_the_dead_edges_are_dead(oracle_mod):
    """What the rows avoid.  At 100 poses / band 5 the last row tile is one row (bw = 65): offset 6 Bb + 5 below a panel's last
    column, which is populated only if that column is element 0 of a 6 x 6 block -- and column 64 st + 63 never is.  Dropping that
    tile changes no bit of any block the gather can return (|I - J| <= Bb), so a row chosen by geometry alone proves nothing.  (A
    dropped tile does leave zeros in Z(W_t, P) at scalar offsets 6 Bb + 5 and beyond; those lie in blocks at distance Bb + 1, which
    no later panel reads and no pair is available for.)
    Offsets just below 6 Bb + 5 are populated only where H itself reaches the full block band in that row (two poses 2 band apart
    sharing a voxel), which is rare: at 300 / band 48 the fourth slice is five indices (bw = 581) and carries data in one panel of
    twenty.  Hence the 300-pose row has band 49, and liveness is asserted from L, never from the geometry."""
    N, band = 100, 5
    row = co.EdgeRow(N, band, "band", dict(loop_frac=0.0), {}, None, ())
    H, _ = _edge_system(oracle_mod, row)
    bw = row.bw(2 * band)
    assert bw == 65
    L, Gs, d = co.ldlt_dense(co.anchor_lower(H, 0), bw)
    table = co.panel_table(6 * N, bw)
    assert not [st for st in co.live_panels(L, bw, "tile") if table[st][4] == bw]   # (a window cut by n ends elsewhere)
    clean = co.selinv_dense(L, Gs, d, bw)
    st = len(Gs) // 2
    assert table[st][4] == bw and co.defect_applies(table[st], "drop_last_tile")
    bad = co.selinv_dense(L, Gs, d, bw, defect=(st, "drop_last_tile"), resume=clean)
    I = np.arange(6 * N) // 6
    near = np.abs(I[:, None] - I[None, :]) <= 2 * band
    assert np.isfinite(np.tril(clean)[near]).all()
    assert np.array_equal(np.tril(clean)[near], np.tril(bad)[near])
