"""The partition of a nested-dissection solve, seen from three sides, and a short numpy restatement of its algebra.  Host only;
used by tests/test_nd_reference_host.py and tests/test_gpu_nd_edges.py.

    plan(...)           what csrc/nd_plan.h makes of a pose graph, through tests/nd_plan_host.cpp (no GPU);
    recover(...)        the same partition rebuilt from what a handle exports: ordering(), info()["nd_sep_poses"] and the 6 x 6
                        block pattern of the exported H;
    Geo                 the table per arc and for the separator that says which masks and stages of the kernels a partition reaches;
    dissect_solve(...)  the algebra of csrc/ldlt_nd.h's header comment in numpy, with one planted defect if asked for -- so that
                        the bars of band_solve_reference can be shown to catch what the GPU rows are there to catch.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
from scipy.linalg import solve_triangular

import band_solve_reference as R

NB = 64  # LVBA_NB
KINDS = ("band", "hubs", "chunks")  # info()["nd_kind"]


@dataclass
class Arc:
    p0: int
    Na: int
    Bb: int
    sep: list            # separator-local poses (positions in the separator's own order) the arc touches, ascending
    owner: int = -1      # the rank that factorises it (-1: not known -- recover() cannot see it)

    def key(self):
        return (self.p0, self.Na, self.Bb, tuple(self.sep))


@dataclass
class Partition:
    perm: np.ndarray     # perm[solver position] = caller's pose
    ps: int
    Ns: int
    BbS: int
    arcs: list = field(default_factory=list)
    kind: int = -1       # index into KINDS (-1: not known)
    Bb_band: int = -1    # of the band ordering the plan started from (plan() only)
    band_is_rcm: int = -1
    perm_band: np.ndarray = None   # that ordering (plan() only)

    def key(self):
        """What recover() and plan() must agree on."""
        return (tuple(int(v) for v in self.perm), self.ps, self.Ns, self.BbS, tuple(a.key() for a in self.arcs))


def adjacency(N, voxel_off, pose_idx):
    """Byte co-visibility matrix [N, N] of a packed problem: two poses that observe one voxel are joined (no diagonal)."""
    adj = np.zeros((N, N), np.uint8)
    voxel_off, pose_idx = np.asarray(voxel_off, np.int64), np.asarray(pose_idx, np.int64)
    for a in range(len(voxel_off) - 1):
        p = pose_idx[voxel_off[a]:voxel_off[a + 1]]
        adj[np.ix_(p, p)] = 1
    np.fill_diagonal(adj, 0)
    return adj


def load(path):
    lib = C.CDLL(path)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    lib.nd_plan_host.restype = C.c_int
    lib.nd_plan_host.argtypes = [np.ctypeslib.ndpointer(np.uint8, flags="C"), C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p,
                                 C.c_int32, i32p, i32p, C.c_int64]
    return lib


def plan(lib, adj, n_ranks=1, chunk_ranks=0):
    """The plan LVBA_SOLVER=nd gives a handle on n_ranks ranks (chunk_ranks: LVBA_ND_CHUNK_RANKS, 0 = unset), or None if the
    planner keeps the band."""
    N = adj.shape[0]
    adj = np.ascontiguousarray(adj, np.uint8)
    head, perm, perm_band = np.zeros(8, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    arcs, off, sep = np.zeros((N, 4), np.int32), np.zeros(N + 1, np.int32), np.zeros(N * N, np.int32)
    rc = lib.nd_plan_host(adj, N, int(n_ranks), int(chunk_ranks), head, perm_band, perm, arcs.reshape(-1), N, off, sep, sep.size)
    assert rc == 0
    if not head[0]:
        return None
    return Partition(perm=perm, ps=int(head[2]), Ns=int(head[3]), BbS=int(head[4]), kind=int(head[1]), Bb_band=int(head[6]),
                     band_is_rcm=int(head[7]), perm_band=perm_band,
                     arcs=[Arc(int(arcs[k, 0]), int(arcs[k, 1]), int(arcs[k, 2]), [int(q) for q in sep[off[k]:off[k + 1]]], int(arcs[k, 3]))
                           for k in range(int(head[5]))])


def block_pattern(H):
    """[N, N] bool: which 6 x 6 blocks of H hold a non-zero."""
    N = H.shape[0] // 6
    return (np.asarray(H).reshape(N, 6, N, 6) != 0).any(axis=(1, 3))


def recover(perm, Ns, H):
    """The partition behind a dissected handle.  Positions [N - Ns, N) of perm are the separator; the arcs are the connected
    components of the rest, which the planner lays out contiguously and largest first; an arc's Bb is the longest of its own
    edges in solver positions, its sep the separator-local poses it touches; BbS is the reach of the separator's graph (direct
    edges + one clique per arc over the separator poses it touches).  Raises if the layout is not of that form."""
    perm = np.asarray(perm, np.int64)
    N = len(perm)
    ps = N - int(Ns)
    pat = block_pattern(H)[np.ix_(perm, perm)]
    np.fill_diagonal(pat, False)
    comp = np.full(ps, -1)
    arcs = []
    for s0 in range(ps):
        if comp[s0] >= 0:
            continue
        members, stack = [], [s0]
        comp[s0] = len(arcs)
        while stack:
            a = stack.pop()
            members.append(a)
            for b in np.nonzero(pat[a, :ps])[0]:
                if comp[b] < 0:
                    comp[b] = len(arcs)
                    stack.append(int(b))
        members.sort()
        p0, Na = members[0], len(members)
        if members != list(range(p0, p0 + Na)):
            raise ValueError(f"arc {len(arcs)} is not contiguous in the ordering")
        i, j = np.nonzero(pat[p0:p0 + Na, p0:p0 + Na])
        sep = sorted(int(q) for q in np.nonzero(pat[p0:p0 + Na, ps:].any(axis=0))[0])
        arcs.append(Arc(p0, Na, int(np.abs(i - j).max()) if len(i) else 0, sep))
    if any(a.Na < b.Na for a, b in zip(arcs, arcs[1:])):
        raise ValueError("the arcs are not laid out largest first")
    fill = pat[ps:, ps:].copy()
    for a in arcs:
        fill[np.ix_(a.sep, a.sep)] = True
    np.fill_diagonal(fill, False)
    i, j = np.nonzero(fill)
    return Partition(perm=perm.astype(np.int32), ps=ps, Ns=int(Ns), BbS=int(np.abs(i - j).max()) if len(i) else 0, arcs=arcs)


# ArcGeo, SepGeo and Geo are COPIES of rules in the solver -- ldlt_use_band and ldlt_ldab (csrc/ldlt_layout.h), ldlt_twist_panels
# and the window of ldlt_solve's geom() (csrc/ldlt.hip), the ldb of nd_alloc (csrc/block_system.hip), the nct of nd_solve
# (csrc/ldlt_nd.h).  Only the separator's Ns and
# BbS and the number of arcs can be asserted against lvba_balm_info.  Whoever changes those rules changes these copies with
# them, or the rows stop reaching the masks and stages they are named for unnoticed.
def use_band(n, bw, band_frac):
    return (bw + NB + 64) < band_frac * n


class ArcGeo:
    def __init__(self, arc, band_frac):
        self.Na, self.Bb, self.nsep, self.owner = arc.Na, arc.Bb, len(arc.sep), arc.owner
        self.n = 6 * arc.Na
        self.rem = self.n % NB                         # rows of the last panel (0: it is full)
        self.bw = 6 * arc.Bb + 5
        self.T = -(-min(self.bw, self.n) // NB)        # tile rows below a panel that the arc's band reaches into
        self.store = "band" if use_band(self.n, self.bw, band_frac) else "dense"
        # tile rows below the first panel that the launches carry (ldlt_solve's geom(): the window is A.bw rows, and a dense store
        # has A.bw = n - 1).  The U role is launched for a panel with T_run >= 2: never for a band-stored arc with T = 1; for a
        # dense-stored one it runs whatever T is, over tiles that hold zeros where the band does not reach
        self.T_run = self.T if self.store == "band" else -(-max(self.n - NB, 0) // NB)
        self.ldb = NB * -(-6 * self.nsep // NB)
        self.nct = self.ldb // NB
        self.pad = self.ldb - 6 * self.nsep

    def __repr__(self):
        return (f"arc(Na={self.Na} n={self.n} rem={self.rem} Bb={self.Bb} bw={self.bw} T={self.T} {self.store} T_run={self.T_run} nsep={self.nsep} "
                f"nct={self.nct} pad={self.pad} owner={self.owner})")


class SepGeo:
    def __init__(self, Ns, BbS, band_frac):
        self.Ns, self.BbS = Ns, BbS
        self.n, self.bw = 6 * Ns, 6 * BbS + 5
        self.store = "band" if use_band(self.n, self.bw, band_frac) else "dense"
        P = (self.n - self.bw) // (2 * NB)
        self.P = P if self.store == "band" and P >= 4 else 0   # panels each end eliminates (0: plain top-down)

    def __repr__(self):
        return f"sep(Ns={self.Ns} n={self.n} BbS={self.BbS} bw={self.bw} {self.store} P={self.P})"


class Geo:
    """The derived table of a partition under a handle's band_frac (0.6 unless configured)."""

    def __init__(self, part, band_frac=0.6):
        self.kind = KINDS[part.kind] if part.kind >= 0 else None
        self.arcs = [ArcGeo(a, band_frac) for a in part.arcs]
        self.sep = SepGeo(part.Ns, part.BbS, band_frac)

    def __repr__(self):
        return f"{self.kind}: " + " ".join(repr(a) for a in self.arcs) + " " + repr(self.sep)


DEFECTS = ("ragged_rows", "pad_column", "far_tiles", "damped_schur", "fp32_Y")


def far_tiles_hold_something(g):
    """Does L(a, a - 2) of an arc with table g hold an entry that is not zero by structure?  T >= 2 is needed but not enough:
    row k of the arc is component k % 6 of its pose and reaches 6 Bb + k % 6 columns to the left, and it needs 64 + k % 64 + 1
    of them to get past the panel before its own.  At bw = 65 the one candidate is the first row of a panel, and 64 a % 6 is
    never 5: the U role's one live row is there and is launched, but holds zeros."""
    return g.T >= 2 and any(6 * g.Bb + k % 6 > NB + k % NB for k in range(2 * NB, g.n))


def defect_applies(defect, g):
    """Can `defect` change anything on an arc with table g (an ArcGeo)?"""
    return {"ragged_rows": g.rem != 0, "pad_column": g.pad > 0, "far_tiles": far_tiles_hold_something(g)}.get(defect, True) and g.nsep > 0


def _forward_near_only(L, E):
    """L^-1 E by 64-row panels in which panel a is updated by L(a, a - 1) alone."""
    n = L.shape[0]
    Y = np.zeros_like(E)
    for k0 in range(0, n, NB):
        k1, j0 = min(k0 + NB, n), max(k0 - NB, 0)
        rhs = E[k0:k1] - L[k0:k1, j0:k0] @ Y[j0:k0]
        Y[k0:k1] = solve_triangular(L[k0:k1, k0:k1], rhs, lower=True, unit_diagonal=True)
    return Y


def dissect_solve(A, b, part, u_applied, defect=None, arc=None):
    """x with A x = b by one level of nested dissection over `part` -- a restatement of the algebra, not of the kernels:
        per arc    A_a = L D L^T (unpivoted), c = L^-1 b_a, Y = L^-1 E_a^T,  S_a = Y^T D^-1 Y,  g_a = Y^T D^-1 c
        separator  S' = S - sum_a S_a,  g' = b_S - sum_a g_a  (in arc order), S' x_S = g' by unpivoted LDL^T
        per arc    x_a = L^-T D^-1 (c - Y x_S)
    A is the damped matrix H + u_applied diag(diag(H)) in the caller's pose order; u_applied is used by "damped_schur" only.
    `defect` plants one fault in arc `arc` (default: the first arc it can change anything on):
        "ragged_rows"   the last n % 64 rows of the arc are left out of Y^T D^-1 Y and Y^T D^-1 c;
        "pad_column"    border column 6 nsep - 1 is dropped from S_a (its row and column are zero);
        "far_tiles"     the border's forward substitution applies only L(a, a - 1) to panel a;
        "damped_schur"  u diag is applied to S - sum S_a instead of to S (every arc; `arc` is ignored);
        "fp32_Y"        Y is rounded to fp32 and back."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"defect must be one of {DEFECTS}")
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    idx = (6 * np.asarray(part.perm, np.int64)[:, None] + np.arange(6)).reshape(-1)
    Ap, bp = A[np.ix_(idx, idx)], b[idx]
    s0 = 6 * part.ps
    if defect is not None and defect != "damped_schur" and arc is None:
        arc = next(k for k, a in enumerate(part.arcs) if defect_applies(defect, ArcGeo(a, 0.6)))
    S = Ap[s0:, s0:].copy()
    if defect == "damped_schur":
        S[np.diag_indices_from(S)] /= 1.0 + u_applied
    gS = bp[s0:].copy()
    kept = []
    for k, a in enumerate(part.arcs):
        r0, n = 6 * a.p0, 6 * a.Na
        cols = (6 * np.asarray(a.sep, np.int64)[:, None] + np.arange(6)).reshape(-1)
        Aa, E = Ap[r0:r0 + n, r0:r0 + n], Ap[r0:r0 + n, s0 + cols]
        L, rcp = R.band_ldlt_numpy(Aa, max(R.bandwidth(Aa), 1))
        c = solve_triangular(L, bp[r0:r0 + n], lower=True, unit_diagonal=True)
        bad = defect if k == arc else None
        Y = _forward_near_only(L, E) if bad == "far_tiles" else solve_triangular(L, E, lower=True, unit_diagonal=True)
        if bad == "fp32_Y":
            Y = Y.astype(np.float32).astype(np.float64)
        live = n - n % NB if bad == "ragged_rows" else n
        Z = Y[:live] * rcp[:live, None]
        Sa, ga = Z.T @ Y[:live], Z.T @ c[:live]
        if bad == "pad_column":
            Sa[-1, :] = 0.0
            Sa[:, -1] = 0.0
        S[np.ix_(cols, cols)] -= Sa
        gS[cols] -= ga
        kept.append((r0, n, cols, L, rcp, c, Y))
    if defect == "damped_schur":
        S[np.diag_indices_from(S)] *= 1.0 + u_applied
    xp = np.empty_like(bp)
    LS, rcpS = R.band_ldlt_numpy(S, max(R.bandwidth(S), 1))
    xS = R.band_ldlt_solve(LS, rcpS, gS)
    xp[s0:] = xS
    for r0, n, cols, L, rcp, c, Y in kept:
        xp[r0:r0 + n] = solve_triangular(L.T, (c - Y @ xS[cols]) * rcp, lower=False, unit_diagonal=True)
    x = np.empty_like(xp)
    x[idx] = xp
    return x


# ------------------------------------------------------------------------------------------------------------ the rows
@dataclass
class RowSpec:
    """make_problem(N, 40 N, band=, seed=, revisit= or loop_frac=0.0) dissected on one rank with LVBA_SOLVER=nd and, where
    chunk_ranks > 0, LVBA_ND_CHUNK_RANKS; reach(geo) is what the row is there for, asserted on the derived table (a Geo)."""
    N: int
    band: int
    seed: int
    revisit: str
    chunk_ranks: int
    kind: str
    arcs: int
    reach: object
    defects: tuple       # the planted defects that can change anything on this row (asserted against defect_applies)

    @property
    def id(self):
        return f"{self.N}-{self.band}-{self.seed}-{self.revisit or 'ring'}-{self.chunk_ranks}"

    def problem_kw(self):
        kw = dict(band=self.band, seed=self.seed)
        kw.update(dict(revisit=self.revisit) if self.revisit else dict(loop_frac=0.0))
        return kw


def _every(g, f):
    return all(f(a) for a in g.arcs)


def _some(g, f):
    return any(f(a) for a in g.arcs)


ALL = DEFECTS
NO_FAR = tuple(d for d in DEFECTS if d != "far_tiles")
ROWS = [
    # T = 1 in dense-stored arcs: has_prev is the only update a panel's border rows get that is not zero -- the U role runs, over
    # tiles of zeros.  A border of one tile column with 16 pad columns, and one of two.  Last panels of 2 and 8 rows.
    RowSpec(300, 4, 5, None, 3, "chunks", 6, lambda g: _every(g, lambda a: a.T == 1 and a.bw == 53 and a.store == "dense" and a.T_run >= 2)
            and _some(g, lambda a: a.nct == 1 and a.pad == 16) and _some(g, lambda a: a.nct == 2)
            and {a.rem for a in g.arcs} == {2, 8} and g.sep.Ns == 40, NO_FAR),
    # bw = 65, one column over a tile, in dense-stored arcs (the U role runs over the whole window; what it adds is zero:
    # far_tiles_hold_something).  A one-tile border with 4 pad columns.  The band-stored neighbour is the last row.
    RowSpec(320, 5, 5, None, 4, "chunks", 6, lambda g: _every(g, lambda a: a.bw == NB + 1 and a.T == 2 and a.store == "dense")
            and _some(g, lambda a: a.nct == 1 and a.pad == 4), NO_FAR),
    # T = 1 in band-stored arcs: the forward substitution runs the Y role only, no U role is launched.  Last panels of 62 rows
    # (nearly full) and of 4
    RowSpec(420, 4, 5, None, 12, "chunks", 7, lambda g: _every(g, lambda a: a.T == 1 and a.store == "band" and a.T_run == 1)
            and {a.rem for a in g.arcs} == {62, 4}, NO_FAR),
    # a hub: arcs of different shape in one solve (border tile columns 2 / 5 / 3), one of them with every panel full
    RowSpec(400, 8, 8, "chords", 0, "hubs", 3, lambda g: _every(g, lambda a: a.T == 2 and a.store == "band")
            and _some(g, lambda a: a.rem == 0) and _some(g, lambda a: a.rem != 0) and len({a.nct for a in g.arcs}) == 3
            and g.sep.store == "dense" and g.sep.P == 0, ALL),
    # T = 4: paired panels and bulk jobs in arcs that carry passengers; a border that fills its tiles exactly (pad 0) and one of
    # 63 poses (6 tile columns)
    RowSpec(360, 16, 5, None, 3, "chunks", 3, lambda g: _every(g, lambda a: a.T == 4 and a.store == "band")
            and _some(g, lambda a: a.pad == 0 and a.nct == 3) and _some(g, lambda a: a.nsep == 63 and a.nct == 6), ALL),
    # dense-stored arcs with a U role; a hub separator larger than any arc
    RowSpec(280, 8, 9, "lot", 0, "hubs", 4, lambda g: _every(g, lambda a: a.T == 2 and a.store == "dense" and a.nct >= 5)
            and g.sep.Ns > max(a.Na for a in g.arcs), ALL),
    # arcs at the planner's minimum (22 poses: nd_build_candidate), a band-stored separator factorised from both ends
    RowSpec(450, 4, 5, None, 14, "chunks", 14, lambda g: _every(g, lambda a: 22 <= a.Na <= 25 and a.T == 1)
            and g.sep.store == "band" and g.sep.P == 4, NO_FAR),
    # bw = 65 in band-stored arcs (320/5's nearest neighbour in N whose arcs are long enough for the band store): the window of a
    # panel is 65 rows, so the U role is launched with one tile, and that tile has one live row
    RowSpec(380, 5, 5, None, 4, "chunks", 6, lambda g: _every(g, lambda a: a.bw == NB + 1 and a.store == "band" and a.T_run == 2)
            and _some(g, lambda a: a.nct == 1 and a.pad == 4), NO_FAR),
]
# three ranks, two arcs: a rank that owns no arc (tests/test_gpu_nd_edges.py::test_a_rank_without_an_arc)
SPARE_RANK_ROW = RowSpec(324, 12, 3, "lot", 0, "hubs", 2, lambda g: sorted(a.owner for a in g.arcs) == [0, 1]
                         and _every(g, lambda a: a.T == 3 and a.store == "band"), ALL)
US = (0.01, 10.0)
ORACLE_MAX = 1.2e-14   # what an unpivoted fp64 LDL^T may leave on a row's system: the figure CAP is derived from (band_solve_reference)


def check_reach(row, part, band_frac=0.6):
    """The row's plan is of the kind it was chosen for and its table reaches what the row is there to reach; returns the table."""
    assert part is not None, (row.id, "the planner kept the band")
    geo = Geo(part, band_frac)
    assert (geo.kind, len(geo.arcs)) == (row.kind, row.arcs), (row.id, geo)
    assert row.reach(geo), (row.id, "the row's table no longer reaches what it is there for", geo)
    applies = tuple(d for d in DEFECTS if any(defect_applies(d, a) for a in geo.arcs))
    assert applies == row.defects, (row.id, applies)
    return geo


def reference(A, b, perm_band):
    """band_solve_reference.reference_solve on the system permuted symmetrically by the plain band ordering (the band LU stays
    as narrow as the graph allows), permuted back."""
    idx = (6 * np.asarray(perm_band, np.int64)[:, None] + np.arange(6)).reshape(-1)
    Ab = A[np.ix_(idx, idx)]
    x = np.empty(len(b), R.LD)
    x[idx] = R.reference_solve(Ab, b[idx], R.bandwidth(Ab))
    return x
