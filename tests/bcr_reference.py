"""The block cyclic reduction of csrc/bcr.hip restated in numpy, with the padding of bcr_assemble_kernel, optional planted
defects, and the bars the reduced-solver tests hold the kernels to.  Host only; used by tests/test_bcr_algorithm.py,
tests/test_bcr_reference_host.py and tests/test_gpu_reduced_solver.py.  The reference (reference_solve) and the two error
measures (errors) are those of tests/band_solve_reference.py.

The scheme (bcr_solve) is the one-launch-per-level form: every even block row's update computed from the level's INPUT coupling
blocks (two L arrays, read one / write the other), both odd neighbours inverted by the even row itself, T1 / T2 / t of an odd row
kept for the back substitution, the levels from stride 1 up to the last one that leaves row 0 alone, then the back substitution
from the largest stride down.  The 64-scalar kernels (bcr_A_kernel / bcr_B_kernel) compute the same quantities in two launches
per level and one L array; as arithmetic they are the same elimination.

The bars of a block-cyclic-reduction solve (within_bars_bcr), on the normwise backward error and on the forward error:
    CAP_BCR  per measure, halfway in decades between the worst error the honest restatement leaves on the two systems of
             tests/test_bcr_reference_host.py (HONEST_WORST) and the least error one odd row's inverse rounded to fp32 leaves
             there over every placement (INV_FP32_LEAST); both measured on the CPU, shown in that test.
    K_BCR    at most K_BCR times the error this restatement leaves on the SAME system, plus 16 eps.  K_BCR is ten times the largest
             ratio (GPU error / restatement error) measured on the MI355X over every row of tests/test_gpu_reduced_solver.py
             (4.53), rounded up to a power of two: 64; the table is in that module's docstring.
The C oracle's unpivoted LDL^T is no yardstick here: explicit inverses of the diagonal blocks cost about two decades in the
backward error (honest restatement 3.2e-15 .. 5.8e-15 against 6.2e-17 .. 8.4e-17 on the two host systems; the forward errors,
1.1e-13 .. 1.7e-13, do not differ).  A fault far smaller than an fp32 rounding -- an inverse off by 1e-12 relative, say -- lands
within a decade or two of the honest range: these bars do not claim to catch it.
"""
import numpy as np

from band_solve_reference import EPS, bandwidth, errors, reference_solve  # noqa: F401  (re-exported for the tests)

# (backward, forward), measured by tests/test_bcr_reference_host.py::test_cap_lies_halfway on the systems 41/4 and 48/7
HONEST_WORST = (5.8e-15, 1.4e-13)     # 48/7, 41/4
INV_FP32_LEAST = (4.0e-9, 3.1e-7)     # both at the last odd row of 41/4: the block row that holds one camera and 26 identity rows
CAP_BCR = tuple(float(np.sqrt(h * d)) for h, d in zip(HONEST_WORST, INV_FP32_LEAST))  # 4.8e-12, 2.1e-10
K_BCR = 64

DEFECTS = ("inv_fp32", "drop_q", "stale_L", "keep_L")


def within_bars_bcr(err, yardstick, measure):
    """The two conditions on one error of a BCR solve; measure 0 = backward, 1 = forward (module docstring)."""
    return err <= CAP_BCR[measure] and err <= K_BCR * yardstick + 16 * EPS


# block_cams, pad and applicable are COPIES of bcr_block_cams, bcr_pad and bcr_applicable (csrc/bcr.hip); whoever changes those
# rules changes these with them.
def block_cams(Bb):
    return 5 if Bb < 5 else Bb


def pad(k):
    return 32 if 6 * k <= 32 else 64


def applicable(M, Bb):
    return 1 <= Bb <= 10 and M >= 8 * block_cams(Bb)


def odd_rows(nb):
    """[(s, i)]: the odd rows i = (2m + 1) s of every level s = 1, 2, 4, .. < nb, in the order they are eliminated."""
    out, s = [], 1
    while s < nb:
        out += [(s, i) for i in range(s, nb, 2 * s)]
        s *= 2
    return out


def placements(nb, need_right=False):
    """The first, a middle and the last odd row (of those with a right neighbour i + s < nb, if asked for)."""
    rows = [(s, i) for s, i in odd_rows(nb) if not need_right or i + s < nb]
    return [rows[0], rows[len(rows) // 2], rows[-1]]


def bcr_solve(D, L, rhs, defect=None, where=None):
    """D [nb, b, b] diagonal blocks, L [nb, b, b] with L[r] = S[r, r - 1] (L[0] unused), rhs [nb, b].  Returns x [nb, b].
    `defect` plants one fault at the odd row where = (s, i) of odd_rows(nb):
        "inv_fp32"  the inverse of that row's diagonal block is rounded to fp32 and back wherever it is used (an odd row is
                    inverted by its left and by its right even neighbour);
        "drop_q"    T2 of that row, the term with L_q^T of its right neighbour q = i + s, is zero although q exists (the back
                    substitution loses the row's coupling to the right);
        "stale_L"   the whole level s reads the L array it should have written (as it stood before the level);
        "keep_L"    at level s the new coupling block of the row without r - 2 s (row 0) is left as the destination array held
                    it instead of being zeroed.  Row 0 has no left neighbour and nobody reads its coupling block: this one is
                    inert, and tests/test_bcr_reference_host.py shows that it is."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"defect must be one of {DEFECTS}")
    nb, b = rhs.shape
    D = D.copy(); rhs = rhs.copy()
    Lbuf = [L.copy(), np.zeros_like(L)]
    cur = 0
    T1 = np.zeros_like(L); T2 = np.zeros_like(L); t = np.zeros_like(rhs)
    s, top = 1, 0
    while s < nb:
        here = where is not None and where[0] == s
        Ls, Ld = Lbuf[cur], Lbuf[cur ^ 1]
        if defect == "stale_L" and here:
            Ls = Ld.copy()

        def inverse(i):
            inv = np.linalg.inv(D[i])
            if defect == "inv_fp32" and here and where[1] == i:
                inv = inv.astype(np.float32).astype(np.float64)
            return inv

        newD, newrhs = {}, {}
        for r in range(0, nb, 2 * s):                       # one "workgroup" per even row; reads only level inputs
            il, ir, q = r - s, r + s, r + 2 * s
            dD = np.zeros((b, b)); dL = np.zeros((b, b)); dr = np.zeros(b)
            if il >= 0:
                inv = inverse(il)
                t1l, t2l, tl = inv @ Ls[il], inv @ Ls[r].T, inv @ rhs[il]
                dD += Ls[r] @ t2l
                dL = Ls[r] @ t1l
                dr += Ls[r] @ tl
            if ir < nb:
                inv = inverse(ir)
                t1r = inv @ Ls[ir]
                t2r = inv @ Ls[q].T if q < nb else np.zeros((b, b))
                if defect == "drop_q" and here and where[1] == ir:
                    t2r = np.zeros((b, b))
                tr = inv @ rhs[ir]
                T1[ir], T2[ir], t[ir] = t1r, t2r, tr        # stored by the LEFT even neighbour
                dD += Ls[ir].T @ t1r
                dr += Ls[ir].T @ tr
            newD[r] = D[r] - dD
            newrhs[r] = rhs[r] - dr
            if il >= 0 and r - 2 * s >= 0:
                Ld[r] = -dL
            elif not (defect == "keep_L" and here):
                Ld[r] = 0.0
        for r in newD:                                       # the even rows' own blocks: nobody else reads them at this level
            D[r], rhs[r] = newD[r], newrhs[r]
        cur ^= 1
        top = s
        s *= 2
    x = np.zeros_like(rhs)
    x[0] = np.linalg.solve(D[0], rhs[0])
    s = top
    while s >= 1:
        for i in range(s, nb, 2 * s):
            x[i] = t[i] - T1[i] @ x[i - s] - (T2[i] @ x[i + s] if i + s < nb else 0.0)
        s //= 2
    return x


def cam_bandwidth(S):
    """Camera half-bandwidth: the largest |I - J| over the non-zero 6 x 6 blocks of S [6M, 6M]."""
    i, j = np.nonzero(S)
    return int(np.abs(i // 6 - j // 6).max()) if len(i) else 0


def assemble(S, b, Bb):
    """The padding of bcr_assemble_kernel: k = block_cams(Bb) cameras per block row, BP = pad(k) scalars; the 6 k' scalars of the
    k' <= k cameras a row really holds (k' < k in a partial last row) come first, the rest of the row is identity with a zero
    right-hand side; L[R] = S[row R, row R - 1] taken from the band (blocks farther than Bb cameras read as zero).
    Returns (D [nb, BP, BP], L [nb, BP, BP], rhs [nb, BP], k)."""
    n = S.shape[0]
    M = n // 6
    k = block_cams(Bb)
    BP = pad(k)
    nb = -(-M // k)
    cam = np.arange(n) // 6
    in_band = np.abs(cam[:, None] - cam[None, :]) <= Bb
    D = np.zeros((nb, BP, BP)); L = np.zeros((nb, BP, BP)); rhs = np.zeros((nb, BP))
    for R in range(nb):
        g0, g1 = 6 * R * k, 6 * min((R + 1) * k, M)
        m = g1 - g0
        D[R] = np.eye(BP)
        D[R, :m, :m] = S[g0:g1, g0:g1]
        rhs[R, :m] = b[g0:g1]
        if R > 0:
            h0 = g0 - 6 * k
            L[R, :m, :6 * k] = np.where(in_band[g0:g1, h0:g0], S[g0:g1, h0:g0], 0.0)
    return D, L, rhs, k


def scatter(xb, M, k):
    """x [6M] out of the padded block rows xb [nb, BP]."""
    x = np.empty(6 * M)
    for R in range(xb.shape[0]):
        g0, g1 = 6 * R * k, 6 * min((R + 1) * k, M)
        x[g0:g1] = xb[R, :g1 - g0]
    return x


def bcr_solve_system(S, b, Bb=None, defect=None, where=None):
    """x with S x = b by the padded block cyclic reduction; S symmetric with camera half-bandwidth <= Bb (default: its own)."""
    S = np.asarray(S, np.float64)
    far = cam_bandwidth(S)
    Bb = far if Bb is None else int(Bb)
    assert far <= Bb and applicable(S.shape[0] // 6, Bb), (far, Bb, S.shape)
    D, L, rhs, k = assemble(S, np.asarray(b, np.float64), Bb)
    return scatter(bcr_solve(D, L, rhs, defect, where), S.shape[0] // 6, k)
