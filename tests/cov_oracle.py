"""Numpy restatement of the covariance path of lvba_balm_covariance (csrc/ldlt_selinv.h) on LAPACK-style lower-band storage:
the one-ended blocked LDL^T in the solver's convention (64-column panels; per panel G = L_PP^-T D_P^-1, d, and L(W, P) stored
below the diagonal block for the window W = rows [k + nbe, min(k + nbe + bw, n))), then the blocked Takahashi recurrence from
the last panel to the first:

    M_P    = L_PP^-1 = D_P G_P^T
    Z(W,P) = -Z(W,W) (L(W,P) M_P)
    Z(P,P) = (G_P - Z(W,P)^T L(W,P)) M_P          (symmetrised)

with Z kept in a band store of the factor's shape (ld = bw + 127 sub-diagonals, as the solver allocates)."""
import numpy as np

NB = 64


def band_store(A, bw, ld=None):
    """lower band of the dense symmetric A: ab[o, c] = A[c + o, c], o <= bw (zeros up to ld)"""
    n = A.shape[0]
    ld = bw + 127 if ld is None else ld
    ab = np.zeros((ld + 1, n))
    for o in range(min(bw, n - 1) + 1):
        ab[o, :n - o] = np.diagonal(A, -o)
    return ab


def _get(ab, r0, r1, c0, c1):
    """dense block A[r0:r1, c0:c1] of the lower store (r >= c entries; zeros beyond the store)"""
    out = np.zeros((r1 - r0, c1 - c0))
    ld = ab.shape[0] - 1
    for c in range(c0, c1):
        for r in range(max(r0, c), r1):
            if r - c <= ld:
                out[r - r0, c - c0] = ab[r - c, c]
    return out


def _get_sym(ab, r0, r1, c0, c1):
    """dense block of the symmetric matrix the lower store holds"""
    out = np.zeros((r1 - r0, c1 - c0))
    ld = ab.shape[0] - 1
    for i, r in enumerate(range(r0, r1)):
        for j, c in enumerate(range(c0, c1)):
            a, b = (r, c) if r >= c else (c, r)
            if a - b <= ld:
                out[i, j] = ab[a - b, b]
    return out


def _put(ab, blk, r0, c0, lower_only=False):
    ld = ab.shape[0] - 1
    for j in range(blk.shape[1]):
        for i in range(blk.shape[0]):
            r, c = r0 + i, c0 + j
            if r >= c and r - c <= ld and (not lower_only or r >= c):
                ab[r - c, c] = blk[i, j]


def panels(n):
    return [(k, min(NB, n - k)) for k in range(0, n, NB)]


def ldlt_band(ab, bw):
    """one-ended blocked LDL^T in place on a copy of ab.  Returns (L store, G list [panel][64 x 64], d [n])"""
    ab = ab.copy()
    n = ab.shape[1]
    d = np.zeros(n)
    Gs = []
    for k, nbe in panels(n):
        A11 = _get(ab, k, k + nbe, k, k + nbe)
        A11 = np.tril(A11) + np.tril(A11, -1).T
        L11 = np.eye(nbe)
        D = np.zeros(nbe)
        W = A11.copy()
        for j in range(nbe):                       # unpivoted scalar LDL^T of the diagonal block
            D[j] = W[j, j]
            L11[j + 1:, j] = W[j + 1:, j] / D[j]
            W[j + 1:, j + 1:] -= np.outer(L11[j + 1:, j], W[j, j + 1:])
        G = np.eye(NB)
        G[:nbe, :nbe] = np.linalg.inv(L11).T / D[None, :]      # G = L11^-T D^-1
        Gs.append(G)
        d[k:k + nbe] = D
        w0, rend = k + nbe, min(k + nbe + bw, n)
        if rend > w0:
            A21 = _get(ab, w0, rend, k, k + nbe)
            L21 = A21 @ G[:nbe, :nbe]
            _put(ab, L21, w0, k)
            C = _get_sym(ab, w0, rend, w0, rend) - (L21 * D[None, :]) @ L21.T
            _put(ab, np.tril(C), w0, w0, lower_only=True)
    return ab, Gs, d


def selinv_band(abL, Gs, d, bw):
    """the panel recurrence: Z (band store of abL's shape) on every stored entry the panels write"""
    n = abL.shape[1]
    Z = np.zeros_like(abL)
    for st in reversed(range(len(Gs))):
        k, nbe = st * NB, min(NB, n - st * NB)
        G = Gs[st][:nbe, :nbe]
        M = d[k:k + nbe, None] * G.T                        # L_PP^-1 = D_P G_P^T
        w0, rend = k + nbe, min(k + nbe + bw, n)
        S = np.zeros((nbe, nbe))
        if rend > w0:
            LW = _get(abL, w0, rend, k, k + nbe)
            ZWW = _get_sym(Z, w0, rend, w0, rend)
            ZWP = -ZWW @ (LW @ M)
            _put(Z, ZWP, w0, k)
            S = ZWP.T @ LW
        ZPP = (G - S) @ M
        ZPP = 0.5 * (ZPP + ZPP.T)
        _put(Z, np.tril(ZPP), k, k, lower_only=True)
    return Z


def band_inverse(A, bw):
    """Z = A^-1 on the band |i - j| <= bw (dense [n, n], NaN outside), through ldlt_band + selinv_band"""
    abL, Gs, d = ldlt_band(band_store(A, bw), bw)
    Z = selinv_band(abL, Gs, d, bw)
    n = A.shape[0]
    out = np.full((n, n), np.nan)
    for o in range(min(bw, n - 1) + 1):
        idx = np.arange(n - o)
        out[idx + o, idx] = Z[o, :n - o]
        out[idx, idx + o] = Z[o, :n - o]
    return out


def anchored(H, anchor):
    """H with pose `anchor`'s rows and columns replaced by the identity's (the gauge held fixed there)"""
    A = H.copy()
    s = slice(6 * anchor, 6 * anchor + 6)
    A[s, :] = 0.0
    A[:, s] = 0.0
    A[s, s] = np.eye(6)
    return A


def inv(A, steps=2):
    """np.linalg.inv with `steps` Newton steps X += X (I - A X): the rounding of the reference itself well below the bars"""
    X = np.linalg.inv(A)
    for _ in range(steps):
        X = X + X @ (np.eye(A.shape[0]) - A @ X)
    return X


def anchored_inverse(H, anchor):
    """inv(H) with the anchor removed, its rows and columns zero: what lvba_balm_covariance returns for an anchor"""
    keep = np.ones(H.shape[0], bool)
    keep[6 * anchor:6 * anchor + 6] = False
    S = np.zeros_like(H)
    S[np.ix_(keep, keep)] = inv(H[np.ix_(keep, keep)])
    return S


def block_bandwidth(H, tol=0.0):
    """pose-block half bandwidth of a 6N x 6N matrix in its own order"""
    N = H.shape[0] // 6
    B = np.abs(H).reshape(N, 6, N, 6).max(axis=(1, 3)) > tol
    i, j = np.nonzero(B)
    return int(np.abs(i - j).max()) if len(i) else 0
