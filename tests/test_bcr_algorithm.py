"""The block cyclic reduction of csrc/bcr.hip as an algorithm, on the CPU (numpy; tests/bcr_reference.py::bcr_solve): the
one-launch-per-level form -- every even block row's update computed from the level's INPUT coupling blocks (two L arrays, read
one / write the other), both odd neighbours inverted by the even row itself, T1 / T2 / t of an odd row kept for the back
substitution, the levels from stride 1 up to the last one that leaves row 0 alone, then the back substitution from the largest
stride down -- against a dense solve.  What the GPU tests hold the kernels to (tests/test_gpu_visual.py,
tests/test_gpu_reduced_solver.py) is this scheme; here its index arithmetic is checked for block-row counts that are not powers
of two, including the ones with a missing right neighbour at several levels."""
import numpy as np
import pytest

from bcr_reference import bcr_solve


@pytest.mark.parametrize("nb", [2, 3, 5, 8, 13, 16, 37, 100, 400])
def test_one_launch_levels_equal_dense_solve(nb):
    rng = np.random.default_rng(nb)
    b = 6
    L = 0.3 * rng.standard_normal((nb, b, b))
    L[0] = 0.0
    A = np.zeros((nb * b, nb * b))
    for r in range(nb):
        M = rng.standard_normal((b, b))
        A[r * b:(r + 1) * b, r * b:(r + 1) * b] = M @ M.T + 4.0 * np.eye(b)
        if r > 0:
            A[r * b:(r + 1) * b, (r - 1) * b:r * b] = L[r]
            A[(r - 1) * b:r * b, r * b:(r + 1) * b] = L[r].T
    assert np.linalg.eigvalsh(A).min() > 0.5
    D = np.stack([A[r * b:(r + 1) * b, r * b:(r + 1) * b] for r in range(nb)])
    rhs = rng.standard_normal((nb, b))
    x = bcr_solve(D, L, rhs)
    ref = np.linalg.solve(A, rhs.reshape(-1)).reshape(nb, b)
    assert np.abs(x - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
