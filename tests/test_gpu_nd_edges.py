"""The damped solve by one level of nested dissection (csrc/nd_plan.h, csrc/ldlt_nd.h, the FwdPassenger roles and ldlt_fwd_kernel of
csrc/ldlt_lookahead.h, the border path of ldlt_solve, nd_alloc in block_system.hip) against a refined reference, at the edges of
its geometry.  tests/test_gpu_nd.py keeps the LM runs and the 1e-8 comparison with a dense solve; this file holds the solve
itself to the bars the band form is held to (tests/test_gpu_band_solver.py).

What is solved and what it is compared with.  `H, g, _ = prob.eval(x0)`, then `dx = prob.solve(u)` on a handle made under
LVBA_SOLVER=nd.  lvba_balm_eval's dense export copies, entry for entry and without arithmetic, the block store `bs.Hblk()` /
`bs.g()` -- on a dissected handle the full lower block triangle in the plan's pose order.  nd_solve (ldlt_nd.h) takes both as
pointers to const and hands them on as such: nd_border_fill_kernel, nd_sep_build_kernel and the fill kernels of the arcs'
ldlt_solve calls read them; everything a solve writes lies elsewhere (the arcs' matrices and workspaces -- their right-hand side b
is ldlt_work_b --, B, Y, S_a, wv, gpart, the separator's Sblk and matrix, d_dx), and lvba_balm_solve does nothing else before the
launches (enqueue_solve -> bs_enqueue_solve: one copy of u).  On several ranks the evaluation all-reduces H and g BEFORE the export.
So A = H + u diag(diag(H)), b = -g built from the EXPORTED H and g is exactly the system the solver was given.  The reference is
band_solve_reference.reference_solve under the plain band ordering (nd_geometry.reference; shown equal to the unpermuted call in
tests/test_nd_reference_host.py).

The bars, on the normwise backward error and on the forward error of every solve: both at most CAP = 5.6e-14, and both at most
K_ND times the error the C oracle's unpivoted LDL^T (oracle.ldlt_solve_dense) leaves on the same system, + 16 eps.  K_ND is ten
times the largest ratio (GPU error / oracle error) measured on the MI355X, rounded up to a power of two -- the rule that gave the
band form K = 8.  The sweep (backward: GPU error, ratio; forward: GPU error, ratio):
    row (N-band-seed-revisit-chunk ranks)   store     u      backward         forward
    300-4-5-ring-3                          default   0.01   3.2e-18  0.32    3.1e-15  0.43
    300-4-5-ring-3                          default   10     6.8e-18  0.45    5.1e-16  0.40
    320-5-5-ring-4                          default   0.01   3.4e-18  0.46    1.9e-15  0.37
    320-5-5-ring-4                          default   10     8.1e-18  0.42    4.4e-16  0.30
    420-4-5-ring-12                         default   0.01   5.0e-18  0.71    1.8e-15  0.47
    420-4-5-ring-12                         default   10     6.2e-18  0.49    4.7e-16  0.55
    400-8-8-chords-0                        default   0.01   7.1e-18  0.61    1.9e-15  0.28
    400-8-8-chords-0                        default   10     6.1e-18  0.35    4.9e-16  0.35
    360-16-5-ring-3                         default   0.01   6.9e-18  0.61    1.5e-15  0.22
    360-16-5-ring-3                         default   10     5.1e-18  0.21    6.2e-16  0.35
    280-8-9-lot-0                           default   0.01   3.4e-18  0.16    1.9e-15  0.21
    280-8-9-lot-0                           default   10     5.8e-18  0.09    7.7e-16  0.18
    450-4-5-ring-14                         default   0.01   5.7e-18  0.65    2.4e-15  0.44
    450-4-5-ring-14                         default   10     1.5e-17  0.91    7.3e-16  0.46
    380-5-5-ring-4                          default   0.01   2.8e-18  0.26    3.8e-15  0.57
    380-5-5-ring-4                          default   10     8.6e-18  0.62    5.7e-16  0.45
    300-4-5-ring-3                          dense     0.01   3.2e-18  0.32    3.1e-15  0.43
    300-4-5-ring-3                          dense     10     6.8e-18  0.45    5.1e-16  0.40
    400-8-8-chords-0                        dense     0.01   7.1e-18  0.61    1.9e-15  0.28
    400-8-8-chords-0                        dense     10     6.1e-18  0.35    4.9e-16  0.35
    320-5-5-ring-4, solves 1 and 3 of three default   0.01   3.4e-18  0.46    1.9e-15  0.37
    320-5-5-ring-4, solve 2 of three        default   10     8.1e-18  0.42    4.4e-16  0.30
    324-12-3-lot-0 on three ranks           default   0.01   3.7e-18  0.11    1.5e-15  0.19
    324-12-3-lot-0 on three ranks           default   10     7.4e-18  0.16    5.5e-16  0.14
    the same dx, single-rank handle's H, g  default   0.01   2.9e-18  0.09    1.4e-15  0.17
    the same dx, single-rank handle's H, g  default   10     9.6e-18  0.21    5.5e-16  0.14
Largest ratio: 0.91 -> K_ND = 16.  The oracle's own errors on these systems: backward 7.0e-18 .. 6.8e-17, forward 8.6e-16 .. 9.2e-15
(280-8-9-lot, u = 0.01); each stays under the 1.2e-14 that CAP is derived from, which every case asserts of its own system.  The
dense store repeats the default store's bits: an arc is factorised top-down in either store, and the tiles the dense store adds
hold zeros (the band form's "notwist" and "dense" rows agree in the same way); that the stores differ is asserted from the
handles' device_bytes.  Every figure is printed by the tests (pytest -s).

The rows: nd_geometry.ROWS, with what each is there to reach.  Before anything is compared a row asserts, from info(), ordering()
and the exported H, that the handle is dissected in the kind and number of arcs the row names, that the partition recovered from
the export IS the plan csrc/nd_plan.h makes on the host (tests/nd_plan_host.cpp), and that the table derived from it
(nd_geometry.Geo) reaches what the row is there for.  A planner change that moves a row fails here; nothing skips.
tests/test_nd_reference_host.py shows on the CPU that the bars catch a ragged last panel dropped from Y^T D^-1 Y, a border
column treated as pad, a forward substitution without its far tiles, damping applied to the Schur complement and an fp32 Y on
these very rows.
"""
import numpy as np
import pytest

import band_solve_reference as R
import nd_geometry as G
from conftest import HostTransport, make_problem, rel
from host_build import build_check

pytestmark = pytest.mark.gpu

BY_ID = {r.id: r for r in G.ROWS}
DENSE_TOO = (G.ROWS[0].id, G.ROWS[3].id)                 # run again with band_frac = 0: every matrix stored dense
CASES = [(r.id, "default") for r in G.ROWS] + [(i, "dense") for i in DENSE_TOO]
REPEAT_ROW = G.ROWS[1]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return G.load(build_check("nd_plan_host", tmp_path_factory.mktemp("nd_plan_host")))


class Row:
    """One (row, store): the dissected handle, the system it exported, its plan and table, and per u the reference and the
    oracle's two errors."""

    def __init__(self, pkg, planner, monkeypatch, spec, store):
        self.spec, self.store = spec, store
        N = spec.N
        d = make_problem(N, 40 * N, **spec.problem_kw())
        self.band_frac = 0.0 if store == "dense" else 0.6
        kw = dict(band_frac=0.0) if store == "dense" else {}
        monkeypatch.delenv("LVBA_ND_CHUNK_RANKS", raising=False)
        monkeypatch.setenv("LVBA_SOLVER", "nond")
        band = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"], **kw)
        try:
            self.band_kind = band.info()["nd_kind"]
            self.Hb, self.gb, self.cb = band.eval(d["poses_init"])
        finally:
            band.close()
        monkeypatch.setenv("LVBA_SOLVER", "nd")
        if spec.chunk_ranks:
            monkeypatch.setenv("LVBA_ND_CHUNK_RANKS", str(spec.chunk_ranks))
        self.prob = pkg.BalmProblem(N, d["voxel_off"], d["pose_idx"], d["clusters"], **kw)
        self.info = self.prob.info()                      # (the plan is made here, under the environment set above)
        self.perm = self.prob.ordering()
        self.H, self.g, self.c = self.prob.eval(d["poses_init"])
        self.plan = G.plan(planner, G.adjacency(N, d["voxel_off"], d["pose_idx"]), 1, spec.chunk_ranks)
        self.sys = {}

    def check_form(self):
        i, spec = self.info, self.spec
        assert self.band_kind == 0
        assert (i["nd_kind"], i["nd_arcs"]) == (G.KINDS.index(spec.kind), spec.arcs), i
        assert self.plan is not None
        assert (i["nd_sep_poses"], i["nd_sep_band_blocks"]) == (self.plan.Ns, self.plan.BbS), (i, self.plan.Ns, self.plan.BbS)
        assert G.recover(self.perm, i["nd_sep_poses"], self.H).key() == self.plan.key()
        geo = G.check_reach(spec, self.plan)              # the plan does not depend on band_frac; the stores do
        if self.store == "dense":
            here = G.Geo(self.plan, self.band_frac)
            assert all(a.store == "dense" for a in here.arcs) and here.sep.store == "dense" and here.sep.P == 0
        # the evaluation does not depend on the order the poses are stored in
        assert rel(self.H, self.Hb) <= 1e-12 and rel(self.g, self.gb) <= 1e-12 and abs(self.c - self.cb) <= 1e-12 * self.cb
        return geo

    def system(self, oracle_mod, u):
        """(A, b, x_ref, yardstick), computed once per u."""
        A = self.H + u * np.diag(np.diag(self.H))
        b = -self.g
        if u not in self.sys:
            x_ref = G.reference(A, b, self.plan.perm_band)
            x_o, rc = oracle_mod.ldlt_solve_dense(A, b)
            assert rc == 0
            self.sys[u] = (x_ref, R.errors(A, b, x_o, x_ref))
        return (A, b) + self.sys[u]


@pytest.fixture(scope="module")
def rows(pkg, planner):
    """rows(monkeypatch, row id, store) -> Row, built on first use; every handle is closed when the module is done."""
    made = {}

    def get(monkeypatch, row_id, store):
        if (row_id, store) not in made:
            made[(row_id, store)] = Row(pkg, planner, monkeypatch, BY_ID[row_id], store)
        return made[(row_id, store)]

    yield get
    for r in made.values():
        r.prob.close()


def _hold(tag, A, b, dx, x_ref, yard):
    assert np.isfinite(dx).all(), tag
    be, fe = R.errors(A, b, dx, x_ref)
    print(f"nd_edges {tag}: backward {be:.3e} (oracle {yard[0]:.3e}, ratio {be / yard[0]:.2f})  "
          f"forward {fe:.3e} (oracle {yard[1]:.3e}, ratio {fe / yard[1]:.2f})")
    assert max(yard) <= G.ORACLE_MAX, (tag, "the row's system is too ill-conditioned for the bars: replace the row", yard)
    assert R.within_bars(be, yard[0], R.K_ND), (tag, "backward", be, yard[0])
    assert R.within_bars(fe, yard[1], R.K_ND), (tag, "forward", fe, yard[1])


@pytest.mark.parametrize("u", G.US)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_dissected_solve_meets_refined_reference(rows, oracle_mod, monkeypatch, case, u):
    c = rows(monkeypatch, *case)
    geo = c.check_form()
    if u == G.US[0]:
        print(f"nd_edges {case[0]} {case[1]}: {geo}")
    A, b, x_ref, yard = c.system(oracle_mod, u)
    if case[1] == "dense":
        # the two handles differ in the arcs' and the separator's stores and workspaces only: more memory exactly where a matrix
        # that was band-stored (400/8: its arcs) is dense now, the same where every one was dense already (300/4)
        more = c.info["device_bytes"] - rows(monkeypatch, case[0], "default").info["device_bytes"]
        assert (more > 0) == any(a.store == "band" for a in geo.arcs), (more, geo)
        assert more >= 0
    dx = c.prob.solve(u)
    _hold(f"{case[0]} {case[1]} u={u}", A, b, dx, x_ref, yard)


def test_repeated_solves_on_one_handle(rows, oracle_mod, monkeypatch):
    """solve(0.01), solve(10), solve(0.01) on the row whose borders have the fewest pad columns: whatever a solve leaves in B, Y,
    S_a, gpart or the arcs' b must not reach the next one -- the first and third results are the same bits, all three hold the bars."""
    c = rows(monkeypatch, REPEAT_ROW.id, "default")
    c.check_form()
    first, second, third = c.prob.solve(0.01), c.prob.solve(10.0), c.prob.solve(0.01)
    assert np.array_equal(first, third)
    for tag, u, dx in (("first", 0.01, first), ("between two solves with 0.01", 10.0, second), ("third", 0.01, third)):
        A, b, x_ref, yard = c.system(oracle_mod, u)
        _hold(f"{REPEAT_ROW.id} u={u} ({tag})", A, b, dx, x_ref, yard)


def test_a_rank_without_an_arc(pkg, planner, oracle_mod, monkeypatch):
    """Three ranks (host threads through tests/host_transport.cpp), two arcs: rank 2 factorises nothing, adds zeros to the
    separator's sum and gets every x_a from the all-reduce.  The ranks agree bitwise; what they exported agrees with the
    single-rank system to 1e-12; rank 0's dx holds the bars on the system the ranks exported -- the one their solve was given."""
    spec, world = G.SPARE_RANK_ROW, 3
    N = spec.N
    d = make_problem(N, 40 * N, **spec.problem_kw())
    off, idx, clu = d["voxel_off"], d["pose_idx"], d["clusters"]
    V = len(off) - 1
    plan = G.plan(planner, G.adjacency(N, off, idx), world, 0)
    G.check_reach(spec, plan)
    monkeypatch.delenv("LVBA_ND_CHUNK_RANKS", raising=False)
    monkeypatch.setenv("LVBA_SOLVER", "nond")
    single = pkg.BalmProblem(N, off, idx, clu)
    try:
        H1, g1, _ = single.eval(d["poses_init"])
    finally:
        single.close()
    monkeypatch.setenv("LVBA_SOLVER", "nd")
    ht = HostTransport(world)

    def rank_main(r):
        a, b = pkg.shard_range(V, r, world)
        prob = pkg.BalmProblem(N, off[a:b + 1], idx[off[a]:off[b]], clu[off[a]:off[b]])
        try:
            ht.attach(prob, r)
            info, perm = prob.info(), prob.ordering()
            H, g, _ = prob.eval(d["poses_init"])
            return dict(info=info, perm=perm, H=H, g=g, dx={u: prob.solve(u) for u in G.US})
        finally:
            prob.close()

    out = ht.run(rank_main)
    r0 = out[0]
    i = r0["info"]
    assert (i["nd_kind"], i["nd_arcs"]) == (G.KINDS.index(spec.kind), spec.arcs) and i["nd_arcs"] < world, i
    assert sorted(a.owner for a in plan.arcs) == [0, 1]
    assert G.recover(r0["perm"], i["nd_sep_poses"], r0["H"]).key() == plan.key()
    for o in out[1:]:
        assert np.array_equal(o["H"], r0["H"]) and np.array_equal(o["g"], r0["g"]) and np.array_equal(o["perm"], r0["perm"])
        for u in G.US:
            assert np.array_equal(o["dx"][u], r0["dx"][u])
    assert rel(r0["H"], H1) <= 1e-12 and rel(r0["g"], g1) <= 1e-12
    # The ranks' H and g are sums in another order than the single-rank handle's (equal to rounding, not bitwise), so rank 0's dx
    # is held twice: on the system the ranks exported -- the one their solve was given -- and on the single-rank handle's.
    for tag, Hx, gx in (("three ranks", r0["H"], r0["g"]), ("three ranks, the single-rank handle's system", H1, g1)):
        for u in G.US:
            A, b = Hx + u * np.diag(np.diag(Hx)), -gx
            x_ref = G.reference(A, b, plan.perm_band)
            x_o, rc = oracle_mod.ldlt_solve_dense(A, b)
            assert rc == 0
            _hold(f"{spec.id} {tag} u={u}", A, b, r0["dx"][u], x_ref, R.errors(A, b, x_o, x_ref))
