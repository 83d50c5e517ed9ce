"""A refined reference for the damped band solve, the two error measures the solver tests hold the kernels to, and a short
numpy LDL^T that can plant a defect (so that the bars can be shown to catch one).  Host only; used by
tests/test_band_solve_reference_host.py, tests/test_gpu_band_solver.py and tests/test_gpu_balm.py::test_solver_schedules.

The bars, on the normwise backward error and on the forward error of a solve (within_bars):
    CAP   at most 5.6e-14: halfway, in decades, between the 2.6e-13 that is the least a pivot reciprocal off by 1e-12 leaves on the
          systems of tests/test_band_solve_reference_host.py and the 1.2e-14 an unpivoted fp64 LDL^T leaves at worst on the systems
          of tests/test_gpu_band_solver.py (cond 2e5 .. 1.4e6).  A dropped tile and an fp32-rounded panel exceed 1e-10.
    K     at most K = 8 times the error of the C oracle's unpivoted LDL^T on the SAME system, plus 16 eps.  K is ten times the
          largest ratio measured on the MI355X over every (row, u, form) of tests/test_gpu_band_solver.py (0.78), rounded up
          to a power of two; the table is in that module's docstring.
    K_ND  the same bar for the solve by nested dissection (tests/test_gpu_nd_edges.py): at most K_ND = 16 times the oracle's error
          on the same system, plus 16 eps -- by the same rule, from the largest ratio of that module's sweep (0.91); its table is in
          that module's docstring.  CAP is the same number for both forms.
"""
import numpy as np
from scipy.linalg import solve_banded, solve_triangular

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CAP = 5.6e-14
K = 8
K_ND = 16
NB = 64  # panel width of band_ldlt_numpy (the kernels' LVBA_NB, but nothing here follows their schedule)


def bandwidth(A):
    """Largest |i - j| with A[i, j] != 0."""
    i, j = np.nonzero(A)
    return int(np.abs(i - j).max()) if len(i) else 0


def _diagonals(A, bw):
    """[2 bw + 1, n] in LAPACK's general band layout: ab[bw + i - j, j] = A[i, j]."""
    n = A.shape[0]
    ab = np.zeros((2 * bw + 1, n))
    for k in range(-bw, bw + 1):  # k > 0: above the diagonal
        d = np.diagonal(A, k)
        if k >= 0:
            ab[bw - k, k:] = d
        else:
            ab[bw - k, :n + k] = d
    return ab


def _band_residual(ab_ld, bw, b_ld, x_ld):
    """b - A x in extended precision, one diagonal at a time (2 bw + 1 vector operations; nothing dense)."""
    n = len(b_ld)
    r = b_ld.copy()
    for k in range(-bw, bw + 1):
        if k >= 0:
            r[:n - k] -= ab_ld[bw - k, k:] * x_ld[k:]
        else:
            r[-k:] -= ab_ld[bw - k, :n + k] * x_ld[:n + k]
    return r


def reference_solve(A, b, bw, max_rounds=8):
    """x (np.longdouble) with A x = b: banded LU with partial pivoting, then iterative refinement with the residual formed in
    np.longdouble over the band, until the correction stops shrinking (two rounds on the systems of these tests).  x is
    accumulated in np.longdouble, so it is not limited by the rounding of an fp64 vector either."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    bw = int(min(bw, n - 1))
    ab = _diagonals(A, bw)
    ab_ld, b_ld = ab.astype(LD), np.asarray(b, np.float64).astype(LD)
    x = solve_banded((bw, bw), ab, np.asarray(b, np.float64)).astype(LD)
    last = np.inf
    for _ in range(max_rounds):
        r = _band_residual(ab_ld, bw, b_ld, x)
        d = solve_banded((bw, bw), ab, r.astype(np.float64))
        size = float(np.abs(d).max())
        if not size < last:  # no longer shrinking: what is left is the rounding of the correction itself
            break
        x += d.astype(LD)
        if size <= 0.0 or size > 0.5 * last:
            break
        last = size
    return x


def errors(A, b, x, x_ref):
    """(normwise backward error |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf), forward error |x - x_ref|_inf / |x_ref|_inf),
    both evaluated in np.longdouble."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    x_ld, b_ld, xr = np.asarray(x).astype(LD), np.asarray(b).astype(LD), np.asarray(x_ref).astype(LD)
    r = np.empty(n, LD)
    norm_a = LD(0)
    for i0 in range(0, n, 256):  # A in extended precision a slab of rows at a time
        Ai = A[i0:i0 + 256].astype(LD)
        r[i0:i0 + 256] = Ai @ x_ld - b_ld[i0:i0 + 256]
        norm_a = max(norm_a, np.abs(Ai).sum(axis=1).max())
    backward = np.abs(r).max() / (norm_a * np.abs(x_ld).max() + np.abs(b_ld).max())
    forward = np.abs(x_ld - xr).max() / np.abs(xr).max()
    return float(backward), float(forward)


def within_bars(err, yardstick, k=K):
    """The two conditions on one error of a solve (module docstring); k: K, or K_ND for a dissected solve."""
    return err <= CAP and err <= k * yardstick + 16 * EPS


DEFECTS = ("drop_tile", "fp32_panel", "rcp_1e-12")


def band_ldlt_numpy(A, bw, defect=None, pivot=None):
    """Blocked unpivoted LDL^T of a symmetric band matrix, 64-column panels, right-looking; returns (L unit lower [n, n],
    rcp [n] = the pivots' reciprocals).  A restatement for the host test, not a mirror of the kernels' schedule.  `defect`
    plants one fault in the MIDDLE panel (panel index n_panels // 2):
        "drop_tile"   its trailing update skips one 64 x 64 tile, the one farthest from the diagonal whose contribution is not
                      zero (the 6 x 6 block structure leaves the corner tile of a band of 65 columns empty, for instance);
        "fp32_panel"  its L panel below the diagonal block is rounded to fp32 and back before it is used and stored;
        "rcp_1e-12"   the reciprocal of its first pivot -- or of pivot `pivot`, an index into the whole matrix -- is off by 1e-12
                      relative (it scales that column of L and is the reciprocal the substitution uses)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"defect must be one of {DEFECTS}")
    W = np.array(A, dtype=np.float64)
    n = W.shape[0]
    L = np.eye(n)
    rcp = np.empty(n)
    bad = ((n + NB - 1) // NB) // 2
    pivot = bad * NB if pivot is None else int(pivot)
    for p, k0 in enumerate(range(0, n, NB)):
        k1 = min(k0 + NB, n)
        r1 = min(k1 + bw, n)  # column k1 - 1 reaches row k1 - 1 + bw
        D = W[k0:k1, k0:k1]
        for j in range(k1 - k0):  # the diagonal block, one pivot at a time (lower triangle)
            rcp[k0 + j] = 1.0 / D[j, j]
            if defect == "rcp_1e-12" and k0 + j == pivot:
                rcp[k0 + j] *= 1.0 + 1e-12
            col = D[j + 1:, j].copy()
            l = col * rcp[k0 + j]
            D[j + 1:, j + 1:] -= np.outer(l, col)
            L[k0 + j + 1:k1, k0 + j] = l
        if r1 == k1:
            continue
        L11 = L[k0:k1, k0:k1]
        Z = solve_triangular(L11, W[k1:r1, k0:k1].T, lower=True, unit_diagonal=True).T  # Z = A21 L11^-T = L21 D
        L21 = Z * rcp[k0:k1]
        if defect == "fp32_panel" and p == bad:
            L21 = L21.astype(np.float32).astype(np.float64)
            Z = L21 / rcp[k0:k1]
        L[k1:r1, k0:k1] = L21
        m = r1 - k1
        nt = (m + NB - 1) // NB
        tile = lambda t: slice(t * NB, min(t * NB + NB, m))
        tiles = [(ti, tj) for ti in range(nt) for tj in range(ti + 1)]  # trailing update, lower tiles of the window
        skip = None
        if defect == "drop_tile" and p == bad:  # farthest from the diagonal first; a tile the band leaves empty is no defect
            skip = next(t for t in sorted(tiles, key=lambda t: (t[1] - t[0], -t[0])) if (Z[tile(t[0])] @ L21[tile(t[1])].T).any())
        for ti, tj in tiles:
            if (ti, tj) != skip:
                W[k1:r1, k1:r1][tile(ti), tile(tj)] -= Z[tile(ti)] @ L21[tile(tj)].T
    return L, rcp


def band_ldlt_solve(L, rcp, b):
    y = solve_triangular(L, np.asarray(b, np.float64), lower=True, unit_diagonal=True)
    return solve_triangular(L.T, y * rcp, lower=False, unit_diagonal=True)
