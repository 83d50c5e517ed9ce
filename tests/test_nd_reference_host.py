"""The rows, the reference and the bars of tests/test_gpu_nd_edges.py, proven on the CPU.

For every row of nd_geometry.ROWS (and the three-rank row): the planner (csrc/nd_plan.h through tests/nd_plan_host.cpp) puts the
row's pose graph into the geometry the row is there to reach; nd_geometry.recover rebuilds exactly that partition from the
planner's ordering and the block pattern of the C oracle's Hessian; on A = H + u diag(diag(H)), u in {0.01, 10}, the C oracle's
unpivoted LDL^T stays within 1.2e-14 in both errors (a condition on the INPUTS: a row that fails it is replaced); the numpy
restatement of the dissection's algebra (nd_geometry.dissect_solve) is inside the bars of band_solve_reference, and the same
restatement with one planted defect is outside them, for every defect that can change anything on the row.

What the planted defects leave (larger of backward and forward error, smallest .. largest over the rows it applies to and the
two u; the oracle 8.5e-16 .. 9.4e-15, the clean restatement 6.4e-16 .. 5.1e-15; every case prints its figures):
    ragged_rows    1.6e-09 .. 2.5e-01        far_tiles      7.2e-07 .. 1.4e-01
    pad_column     3.0e-07 .. 2.5e-01        damped_schur   7.9e-04 .. 5.4e-03
    fp32_Y         1.7e-10 .. 2.2e-08
Which defect applies where: "ragged_rows" needs an arc with n % 64 != 0, "pad_column" one whose border does not fill its tiles,
"far_tiles" one in which L(a, a - 2) holds something -- T >= 2 is needed but not enough: at bw = 65 (the 320/5 and 380/5 rows) the
far tile's one live row is zero by the 6 x 6 block structure (nd_geometry.far_tiles_hold_something), so those rows are there for
the launch and its mask, and the defect is studied on the rows with T = 2 at bw = 101 and above.

The U role is launched by the STORE's window (nd_geometry.ArcGeo.T_run), not by the graph's band: a dense-stored arc runs it over
its whole trailing window, where the tiles the band does not reach hold zeros.  So 300/4 and 320/5 (dense-stored arcs) reach the
masks of the border and of the last panel, 420/4 (band-stored, T = 1) the forward substitution without a U role, and 380/5 --
320/5's nearest neighbour in N whose arcs are long enough for the band store -- the U role whose one tile has one live row.

Two rows are not the ones first probed: 280/8 'lot' runs with seed 9 and the three-rank row with 324 poses, because at seed 3 /
320 poses the oracle's own forward error at u = 0.01 is 1.7e-14 / 1.3e-14, over the 1.2e-14 the bars assume of the inputs.
"""
import numpy as np
import pytest

import band_solve_reference as R
import nd_geometry as G
from conftest import make_problem
from host_build import build_check

ROWS = G.ROWS + [G.SPARE_RANK_ROW]
_CACHE = {}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return G.load(build_check("nd_plan_host", tmp_path_factory.mktemp("nd_plan_host")))


def _row(planner, oracle_mod, row):
    """(partition, table, H, g) of a row: built once and left unchanged."""
    if row.id not in _CACHE:
        d = make_problem(row.N, 40 * row.N, **row.problem_kw())
        part = G.plan(planner, G.adjacency(row.N, d["voxel_off"], d["pose_idx"]), 3 if row is G.SPARE_RANK_ROW else 1, row.chunk_ranks)
        geo = G.check_reach(row, part)
        H, g, _ = oracle_mod.COracle(row.N, d["voxel_off"], d["pose_idx"], d["clusters"]).eval_dense(d["poses_init"])
        _CACHE[row.id] = (part, geo, np.array(H), g)
    return _CACHE[row.id]


def _system(planner, oracle_mod, row, u):
    """(A, b, x_ref, the oracle's two errors), once per (row, u)."""
    part, _, H, g = _row(planner, oracle_mod, row)
    if (row.id, u) not in _CACHE:
        A, b = H + u * np.diag(np.diag(H)), -g
        x_ref = G.reference(A, b, part.perm_band)
        x_o, rc = oracle_mod.ldlt_solve_dense(A, b)
        assert rc == 0
        _CACHE[(row.id, u)] = (A, b, x_ref, R.errors(A, b, x_o, x_ref))
    return _CACHE[(row.id, u)]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_row_lands_where_it_is_meant_to_and_recover_finds_the_plan(planner, oracle_mod, row):
    part, geo, H, _ = _row(planner, oracle_mod, row)      # (_row asserts the reach)
    print(f"nd row {row.id}: Bb_band {part.Bb_band} ({'rcm' if part.band_is_rcm else 'natural'}) {geo}")
    assert sorted(part.perm.tolist()) == list(range(row.N)) and part.ps + part.Ns == row.N
    got = G.recover(part.perm, part.Ns, H)
    assert got.key() == part.key()
    # a separator pose moved to the front is no longer the planner's layout: recover refuses it or returns another partition
    moved = np.concatenate([part.perm[-1:], part.perm[:-1]])
    try:
        assert G.recover(moved, part.Ns, H).key() != part.key()
    except ValueError:
        pass


def test_permuted_reference_equals_the_unpermuted_one(planner, oracle_mod):
    """280/8/9 'lot', whose band ordering is rcm_order's: the reference computed under that ordering and permuted back against
    reference_solve on the system as it stands (band LU over nearly the whole matrix), to the rounding of the refinement."""
    row = G.ROWS[5]
    part = _row(planner, oracle_mod, row)[0]
    assert part.band_is_rcm == 1 and not np.array_equal(part.perm_band, np.arange(row.N))
    for u in G.US:
        A, b, x_ref, _ = _system(planner, oracle_mod, row, u)
        plain = R.reference_solve(A, b, R.bandwidth(A))
        diff = float(np.abs(x_ref - plain).max() / np.abs(plain).max())
        print(f"nd reference 280/8 u={u}: permuted against plain {diff:.3e}")
        assert x_ref.dtype == R.LD and diff <= 1e-15


@pytest.mark.parametrize("u", G.US)
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_restatement_meets_the_bars_and_every_planted_defect_does_not(planner, oracle_mod, row, u):
    part = _row(planner, oracle_mod, row)[0]
    A, b, x_ref, yard = _system(planner, oracle_mod, row, u)
    print(f"nd host {row.id} u={u}: oracle {yard[0]:.3e} {yard[1]:.3e}")
    assert max(yard) <= G.ORACLE_MAX, "the row's system is too ill-conditioned for the bars: replace the row"
    got = R.errors(A, b, G.dissect_solve(A, b, part, u), x_ref)
    print(f"nd host {row.id} u={u}: clean {got[0]:.3e} {got[1]:.3e}")
    for e, y in zip(got, yard):
        assert R.within_bars(e, y), (got, yard)
    for defect in row.defects:
        bad = R.errors(A, b, G.dissect_solve(A, b, part, u, defect), x_ref)
        print(f"nd host {row.id} u={u}: {defect} {bad[0]:.3e} {bad[1]:.3e}")
        assert max(bad) > R.CAP, (defect, bad)
        assert not (R.within_bars(bad[0], yard[0]) and R.within_bars(bad[1], yard[1])), (defect, bad, yard)
