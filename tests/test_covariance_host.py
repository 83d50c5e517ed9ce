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
