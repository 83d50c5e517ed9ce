"""Numpy restatement of the covariance path of lvba_balm_covariance (csrc/ldlt_selinv.h) on LAPACK-style lower-band storage:
the one-ended blocked LDL^T in the solver's convention (64-column panels; per panel G = L_PP^-T D_P^-1, d, and L(W, P) stored
below the diagonal block for the window W = rows [k + nbe, min(k + nbe + bw, n))), then the blocked Takahashi recurrence from
the last panel to the first:

    M_P    = L_PP^-1 = D_P G_P^T
    Z(W,P) = -Z(W,W) (L(W,P) M_P)
    Z(P,P) = (G_P - Z(W,P)^T L(W,P)) M_P          (symmetrised)

with Z kept in a band store of the factor's shape (ld = bw + 127 sub-diagonals, as the solver allocates).

Below that: the same recurrence on dense arrays with the kernels' tile and slice geometry (panel_table, selected_inverse), planted
defects, the error metric of the GPU tests (worst), the rows of the edge tests (EDGE_ROWS) and their bars (within_bars)."""
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


# ---------------------------------------------------------------------------------------------------------------------------------
# The same recurrence on dense [n, n] arrays by block slices: fast enough (n = 2160 in under 2 s) to be the yardstick of the GPU
# edge tests (tests/test_gpu_covariance_edges.py), with the kernels' tile / slice geometry and planted defects.

EPS = float(np.finfo(np.float64).eps)
KSMAX = 8   # LVBA_SI_KSMAX


# panel_table is a COPY of the rule in ldlt_selinv (ldlt.hip): the window of each panel, its row tiles and the split of the inner
# dimension into slices.  Nothing of it is exported, so it cannot be asserted against the handle.  Whoever changes that rule changes
# this copy with it, or the rows of the edge tests stop reaching the tiles and slices they are named for unnoticed.
def panel_table(n, bw):
    """per panel (k, nbe, w0, rend, nw, T, KS, ksz): columns [k, k + nbe), window rows [w0, rend), nw of them in T row tiles of
    64, the inner dimension in KS slices of ksz indices (the last one shorter)"""
    out = []
    for k in range(0, n, NB):
        nbe = min(NB, n - k)
        w0, rend = k + nbe, min(k + nbe + bw, n)
        nw = max(rend - w0, 0)
        T = (nw + 63) // 64
        KS, ksz = 1, nw
        if T > 0:
            ks = max(1, min(KSMAX, nw // 128, 256 // T))
            ksz = ((nw + ks - 1) // ks + 63) // 64 * 64
            KS = (nw + ksz - 1) // ksz
        out.append((k, nbe, w0, rend, nw, T, KS, ksz))
    return out


def last_tile_rows(row):
    """window-relative rows of the last row tile if it is a partial one, else None"""
    nw, T = row[4], row[5]
    return slice(64 * (T - 1), nw) if T > 0 and nw % 64 else None


def slice_rows(row, s):
    """window-relative inner indices of slice s"""
    nw, ksz = row[4], row[7]
    return slice(s * ksz, min((s + 1) * ksz, nw))


DEFECTS = ("drop_last_tile", "drop_last_slice", "drop_mid_slice", "fp32_x", "anchor_row_kept")


def defect_applies(row, kind):
    """does panel `row` of panel_table have the feature that `kind` breaks (anchor_row_kept is not a panel's: see anchor_lower)"""
    T, KS = row[5], row[6]
    return {"drop_last_tile": last_tile_rows(row) is not None, "drop_last_slice": KS > 1, "drop_mid_slice": KS > 2,
            "fp32_x": T > 0}[kind]


def anchor_lower(H, c0, row_kept=False):
    """What ldlt_anchor_kernel leaves of H (symmetric; only its lower triangle is read, as the factorisation reads it) for an
    anchor whose block starts at scalar column c0: columns c0 .. c0 + 5 below the diagonal and rows c0 .. c0 + 5 left of it
    become the identity's.  row_kept (defect anchor_row_kept): the rows are not cleared.  Returns the symmetric matrix whose lower
    triangle that is.  (At c0 = 0 there is nothing left of the block, and the defect changes nothing.)"""
    Lo = np.tril(H)
    Lo[c0:, c0:c0 + 6] = 0.0
    if not row_kept:
        Lo[c0:c0 + 6, :c0] = 0.0
    Lo[np.arange(c0, c0 + 6), np.arange(c0, c0 + 6)] = 1.0
    return Lo + np.tril(Lo, -1).T


def ldlt_dense(A, bw):
    """ldlt_band on dense arrays: (L [n, n] holding L(W, P) below each diagonal block, zero elsewhere; G list; d).  Entries of A
    beyond the band |i - j| <= bw are not read."""
    n = A.shape[0]
    i = np.arange(n)
    W = np.where(np.abs(i[:, None] - i[None, :]) <= bw, A, 0.0)
    W = np.tril(W) + np.tril(W, -1).T
    L = np.zeros((n, n))
    d = np.zeros(n)
    Gs = []
    for k, nbe in panels(n):
        P = slice(k, k + nbe)
        B = W[P, P].copy()
        L11 = np.eye(nbe)
        D = np.zeros(nbe)
        for j in range(nbe):                       # unpivoted scalar LDL^T of the diagonal block
            D[j] = B[j, j]
            L11[j + 1:, j] = B[j + 1:, j] / D[j]
            B[j + 1:, j + 1:] -= np.outer(L11[j + 1:, j], B[j, j + 1:])
        G = np.eye(NB)
        G[:nbe, :nbe] = np.linalg.inv(L11).T / D[None, :]
        Gs.append(G)
        d[P] = D
        w0, rend = k + nbe, min(k + nbe + bw, n)
        if rend > w0:
            Wn = slice(w0, rend)
            L21 = W[Wn, P] @ G[:nbe, :nbe]
            L[Wn, P] = L21
            W[Wn, Wn] -= (L21 * D[None, :]) @ L21.T
    return L, Gs, d


def selinv_dense(L, Gs, d, bw, defect=None, resume=None):
    """selinv_band on dense arrays, in the kernels' order of operations: per panel X = sum over the inner slices s (in order) of
    Z(W, W_s) L(W_s, P), then Z(W, P) = -X M_P, Q = Z(W, P)^T L(W, P), Z(P, P) = (G_P - Q) M_P symmetrised.  Z: [n, n], lower
    triangle, NaN where no panel wrote -- a read of such an entry would poison the result, so a finite result also shows that
    Z(W, W) is only read where the store holds it.

    defect = (panel index, kind) plants one fault in stage 0 of that panel:
        "drop_last_tile"   the rows of X of the last, partial row tile are zero (the tile's workgroups did nothing);
        "drop_last_slice"  the last inner slice is left out of the sum;
        "drop_mid_slice"   slice KS // 2 is left out of the sum;
        "fp32_x"           X is rounded to fp32 and back.
    ("anchor_row_kept" is planted in the matrix: anchor_lower.)  resume: the clean result of the same factor -- the panels after
    the defective one are taken from it instead of being computed again (they do not depend on the defect)."""
    n = L.shape[0]
    table = panel_table(n, bw)
    Z = np.full((n, n), np.nan) if resume is None else resume.copy()
    for st in reversed(range(len(Gs) if resume is None else defect[0] + 1)):
        k, nbe, w0, rend, nw, T, KS, ksz = table[st]
        kind = defect[1] if defect is not None and defect[0] == st else None
        if kind is not None:
            if kind not in DEFECTS[:4]:
                raise ValueError(f"defect kind must be one of {DEFECTS[:4]}")
            if not defect_applies(table[st], kind):
                raise ValueError(f"panel {st} has nothing for {kind} to break: {table[st]}")
        P = slice(k, k + nbe)
        G = Gs[st][:nbe, :nbe]
        M = d[P, None] * G.T                                # L_PP^-1 = D_P G_P^T
        Q = np.zeros((nbe, nbe))
        if nw > 0:
            Wn = slice(w0, rend)
            LW = L[Wn, P]
            Zl = Z[Wn, Wn]
            ZWW = np.tril(Zl) + np.tril(Zl, -1).T
            skip = {"drop_last_slice": KS - 1, "drop_mid_slice": KS // 2}.get(kind, -1)
            X = np.zeros((nw, nbe))
            for s in range(KS):
                if s != skip:
                    sl = slice_rows(table[st], s)
                    X += ZWW[:, sl] @ LW[sl]
            if kind == "drop_last_tile":
                X[last_tile_rows(table[st])] = 0.0
            if kind == "fp32_x":
                X = X.astype(np.float32).astype(np.float64)
            ZWP = -(X @ M)
            Z[Wn, P] = ZWP
            Q = ZWP.T @ LW
        ZPP = (G - Q) @ M
        Z[P, P] = np.tril(0.5 * (ZPP + ZPP.T))
    return Z


def sym_band(Zl, bw):
    """the symmetric dense [n, n] of selinv_dense's lower triangle, NaN outside the band |i - j| <= bw"""
    i = np.arange(Zl.shape[0])
    Zl = np.where(i[:, None] - i[None, :] <= bw, np.tril(Zl), np.nan)
    return Zl + np.tril(Zl, -1).T


def selected_inverse(A, bw, defect=None):
    """(Z, L): Z = A^-1 on the band |i - j| <= bw as a symmetric dense [n, n] (NaN outside the band), through ldlt_dense +
    selinv_dense; L as ldlt_dense returns it, for the callers' liveness tests"""
    L, Gs, d = ldlt_dense(A, bw)
    return sym_band(selinv_dense(L, Gs, d, bw, defect), bw), L


def live_panels(L, bw, feature):
    """indices of the panels whose last partial row tile ("tile"), last inner slice of KS > 1 ("slice") or middle slice of
    KS > 2 ("mid") holds a non-zero of L(W, P): only there does that tile or slice carry data into the result"""
    out = []
    for st, row in enumerate(panel_table(L.shape[0], bw)):
        k, nbe, w0, rend, nw, T, KS, ksz = row
        if feature == "tile":
            sl = last_tile_rows(row)
        else:
            sl = slice_rows(row, KS - 1 if feature == "slice" else KS // 2) if KS > (1 if feature == "slice" else 2) else None
        if sl is not None and L[w0:rend, k:k + nbe][sl].any():
            out.append(st)
    return out


def blocks_of(Z, pairs, anchor=None, order=None):
    """(diag [N, 6, 6], pair blocks [K, 6, 6]) of the dense Z as lvba_balm_covariance returns them: caller pose a sits at block
    order[a] of Z (None: Z is in the caller's order), and the anchor's blocks are zeros"""
    N = Z.shape[0] // 6
    o = np.arange(N) if order is None else np.asarray(order)
    B = Z.reshape(N, 6, N, 6)
    diag = np.stack([B[o[a], :, o[a], :] for a in range(N)])
    blk = np.stack([B[o[a], :, o[b], :] for a, b in pairs]) if len(pairs) else np.zeros((0, 6, 6))
    if anchor is not None:
        diag[anchor] = 0.0
        for q, (a, b) in enumerate(pairs):
            if a == anchor or b == anchor:
                blk[q] = 0.0
    return diag, blk


def _worst_ratio(err, den):
    """largest err / den (0 for none); a NaN counts as infinite (max() would drop it)"""
    if err.size == 0:
        return 0.0
    r = err / den
    return float("inf") if np.isnan(r).any() else float(r.max())


def worst(S, diag, pairs, blocks, avail):
    """max over poses of |dSigma_i|_F / |Sigma_i|_F and over available pairs of |dSigma_ij|_F / sqrt(|Sigma_ii|_F |Sigma_jj|_F);
    where the reference block is zero (an anchor's) the block must be zero too"""
    N = diag.shape[0]
    B = S.reshape(N, 6, N, 6)
    fro = lambda x: np.sqrt((x * x).sum(axis=(1, 2)))
    ar = np.arange(N)
    Sd = B[ar, :, ar, :]
    nd = fro(Sd)
    assert np.all(diag[nd == 0] == 0.0)
    wd = _worst_ratio(fro(diag - Sd)[nd > 0], nd[nd > 0])
    P = np.asarray(pairs, np.int64).reshape(-1, 2)
    av = np.asarray(avail, bool)
    P, blk = P[av], np.asarray(blocks)[av]
    den = np.sqrt(nd[P[:, 0]] * nd[P[:, 1]])
    assert np.all(blk[den == 0] == 0.0)
    wp = _worst_ratio(fro(blk - B[P[:, 0], :, P[:, 1], :])[den > 0], den[den > 0])
    return wd, wp


# ---------------------------------------------------------------------------------------------------------------------------------
# The rows of the edge tests (tests/test_covariance_host.py shows them live on the CPU, tests/test_gpu_covariance_edges.py runs
# them): make_problem(N, 40 N, band=band, seed=5, **problem) into BalmProblem(.., **handle).  Block half-bandwidth Bb = 2 band in
# band storage, bw = 6 Bb + 5; dense storage: bw = n - 1.  reach: asserted on panel_table(n, bw); live: the features (live_panels)
# that must carry non-zero data in at least one panel.  A 64-column panel never ends on element 0 of a 6 x 6 block, so band offset
# 6 Bb + 5 is never populated below a panel: a last tile of one row (band 5 of the N = 100 row) multiplies zeros, a last slice of
# five indices (band 48 of the N = 300 row) does in nearly every panel, and so does every far slice of a dense store over a banded
# H (no fill outside the band) -- hence loop closures on the two large dense rows.
class EdgeRow:
    def __init__(self, N, band, store, problem, handle, reach, live):
        self.N, self.band, self.store, self.problem, self.handle, self.reach, self.live = N, band, store, problem, handle, reach, live
        self.n = 6 * N
        self.id = f"{N}-{band}-{store}"

    def bw(self, band_blocks):
        return 6 * band_blocks + 5 if self.store == "band" else self.n - 1


_T = lambda t: [r[5] for r in t]
_KS = lambda t: [r[6] for r in t]
_NOLOOP = dict(loop_frac=0.0)
EDGE_ROWS = [
    # n = 66: a second panel of 2 columns; the first panel's window is one tile of 2 rows
    EdgeRow(11, 3, "dense", {}, {}, lambda t: len(t) == 2 and t[1][1] == 2 and t[0][4:7] == (2, 1, 1), ("tile",)),
    # bw = 29 < 64: one row tile with rlim = 29 everywhere, last panel 32 columns
    EdgeRow(48, 2, "band", _NOLOOP, {}, lambda t: t[0][4] == 29 and max(_T(t)) == 1 and max(r[4] for r in t) == 29 and t[-1][1] == 32,
            ("tile",)),
    # n = 6 * 64: every panel full; bw = 149, T steps 3, 2, 1, 0 (the default band_frac would pick dense)
    EdgeRow(64, 12, "band", _NOLOOP, dict(band_frac=0.8), lambda t: all(r[1] == 64 for r in t) and t[0][4] == 149 and _T(t) == [3, 3, 3, 2, 1, 0],
            ("tile",)),
    # bw = 77: a second tile of 13 rows
    EdgeRow(100, 6, "band", _NOLOOP, {}, lambda t: t[0][4:6] == (77, 2) and t[0][4] - 64 == 13, ("tile",)),
    # bw = 593: T = 10, KS = 4 slices of 192, the fourth 17 long; KS falls 4 -> 1 where n cuts the window
    EdgeRow(300, 49, "band", _NOLOOP, {}, lambda t: t[0][4:] == (593, 10, 4, 192) and 593 - 3 * 192 == 17 and set(_KS(t)) == {4, 3, 2, 1},
            ("tile", "slice", "mid")),
    # n = 2160, bw = 329: T = 6, KS = 2 slices of 192, the second 137 = 2 * 64 + 9 long
    EdgeRow(360, 27, "band", _NOLOOP, {}, lambda t: t[0][4:] == (329, 6, 2, 192) and 329 - 192 == 2 * 64 + 9, ("tile", "slice")),
    # T = 33 > 32: 256 / T = 7 binds (nw / 128 = 16); ksz = 320; KS reaches 8 on later panels
    EdgeRow(360, 27, "dense", {}, {}, lambda t: t[0][5:] == (33, 7, 320) and 256 // 33 == 7 < t[0][4] // 128 and max(_KS(t)) == 8,
            ("tile", "slice", "mid")),
    EdgeRow(300, 49, "dense", {}, {}, lambda t: t[0][5:] == (28, 7, 256) and max(_KS(t)) == 8, ("tile", "slice", "mid")),
]


def plant_sites(L, bw):
    """{kind: panels} where the host test plants each stage-0 defect: the first and the middle of the panels in which the feature
    is live (fp32_x: of the panels that have a window)"""
    table = panel_table(L.shape[0], bw)
    pick = lambda v: sorted({v[0], v[len(v) // 2]}) if v else []
    return {"drop_last_tile": pick(live_panels(L, bw, "tile")), "drop_last_slice": pick(live_panels(L, bw, "slice")),
            "drop_mid_slice": pick(live_panels(L, bw, "mid")), "fp32_x": pick([st for st, r in enumerate(table) if r[5] > 0])}


# The bars on the two figures of worst() (within_bars), for the kernels against the yardstick = the same figure of the fp64
# restatement (selected_inverse) on the same matrix in the same order:
#   K    at most K = 16 times the yardstick, plus 16 eps.  K is ten times the largest ratio (GPU error / yardstick) measured on the
#        MI355X over every (row, anchor) of tests/test_gpu_covariance_edges.py (0.83), rounded up to a power of two; the table is in
#        that module's docstring.
#   CAP  at most 3.0e-10 = 64 times the largest yardstick of that sweep (4.73e-12: matrices of cond 1e6 .. 1e8).  The multiple is
#        4 K: four times what the K bar allows at the worst yardstick, and a tenth of the least an fp32-rounded stage-0 product of
#        one single panel leaves on the diagonal blocks of these rows (3.1e-9, tests/test_covariance_host.py).
# Both are conditions: tests/test_covariance_host.py shows every planted defect outside them.
CAP = 3.0e-10
K = 16


def within_bars(err, yardstick):
    """err: a figure of worst() for the kernels; yardstick: the same figure for the fp64 restatement (selected_inverse) on the same
    matrix in the same order"""
    return err <= CAP and err <= K * yardstick + 16 * EPS
