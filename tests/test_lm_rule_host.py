"""CPU tests of the LM damping rule (csrc/lm_rule.h compiled for the host): its decisions, u and v against the control flow of
oracle.balm_oracle.damping_iter and of tests/posegraph_oracle.py on scripted and real cost sequences, bit for bit; flagged rows;
max_iter = 0."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import posegraph_cases as pgc
import posegraph_oracle as pg
from host_build import build_check
from oracle import balm_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, FACTORIZATION, NONFINITE = 0, 1, 2      # LVBA_OK, LVBA_NUM_* of include/lvba_hip.h


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    lib = ctypes.CDLL(build_check("lm_rule_check", tmp_path_factory.mktemp("lm_rule"), flags=("-O2", "-std=c++17", "-Wall", "-Werror")))
    lib.lmr_replay.argtypes = [ctypes.c_int, np.ctypeslib.ndpointer(np.float64, flags="C"), ctypes.c_double, ctypes.c_double, ctypes.c_double,
                               ctypes.c_int, ctypes.c_int, np.ctypeslib.ndpointer(np.int32, flags="C"), np.ctypeslib.ndpointer(np.float64, flags="C")]
    lib.lmr_replay.restype = ctypes.c_int

    def replay(rows, rel_tol, max_iter, stop_on_reject, u0=0.01, v0=2.0):
        """rows of (r1, r2, q1, flagged) -> (done before any step, per row dict(accepted, evaluated, status, done, u, v, q))"""
        a = np.ascontiguousarray(np.array(rows, np.float64).reshape(-1, 4))
        io, do = np.zeros((len(a), 4), np.int32), np.zeros((len(a), 3))
        done0 = lib.lmr_replay(len(a), a, u0, v0, rel_tol, max_iter, int(stop_on_reject), io, do)
        assert done0 in (0, 1)      # (-1: a row's iter is not its index)
        return bool(done0), [dict(accepted=int(i[0]), evaluated=int(i[1]), status=int(i[2]), done=bool(i[3]), u=float(d[0]), v=float(d[1]),
                                  q=float(d[2])) for i, d in zip(io, do)]
    return replay


def _same(got, want, ended=True):
    """the rule's rows against an oracle's rows (accepted, evaluated, u, v, r1, r2): equal decisions, u and v equal as doubles, and
    done on the oracle's last row only (ended = False: on none)"""
    assert len(got) == len(want) >= 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["accepted"] == int(w["accepted"]) and g["evaluated"] == int(w["evaluated"]), k
        assert g["v"] == w["v"] and g["u"] == w["u"], (k, g["u"], w["u"])
        assert g["done"] == (ended and k == len(want) - 1), k


def _rows(trace):
    return [(w["residual1"], w["residual2"], w["q1"], 0.0) for w in trace]


def _balm_script(costs, max_iter=None, rel_tol=1e-6):
    """oracle.balm_oracle.damping_iter on one pose with a fixed H and g, the trial costs scripted (the start costs 1.0) and the
    current cost the last accepted one: its trace as dicts"""
    H, g = np.diag([4.0, 5.0, 6.0, 7.0, 8.0, 9.0]), np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.2])
    todo, state = list(costs), dict(trial=1.0)

    def cost_fn(x):
        state["trial"] = todo.pop(0)
        return state["trial"]

    # (an evaluation happens at the start and after an acceptance: the last trial cost is then the current point's)
    _, trace = bo.damping_iter(SimpleNamespace(n_voxels=3), np.r_[np.eye(3).reshape(9), 0.0, 0.0, 0.0], max_iter=max_iter or len(costs),
                               rel_tol=rel_tol, eval_fn=lambda x: (H, g, state["trial"]), cost_fn=cost_fn, solve_fn=np.linalg.solve)
    return [dict(accepted=r.accepted, evaluated=r.evaluated, u=r.u, v=r.v, residual1=r.residual1, residual2=r.residual2, q1=r.q1) for r in trace]


REJECT_CHAIN = [1.2, 1.5, 3.0, 0.8, 0.9, 0.7, 0.6999, 0.69]


def test_accepted_steps_equal_the_balm_oracle(rule):
    t = _balm_script([0.9, 0.5, 0.45, 0.449, 0.448999999])
    assert [r["accepted"] for r in t] == [True] * 5
    _same(rule(_rows(t), 1e-6, 5, True)[1], t)


def test_reject_chain_equals_the_balm_oracle(rule):
    t = _balm_script(REJECT_CHAIN)
    assert [int(r["accepted"]) for r in t] == [0, 0, 0, 1, 0, 1, 1, 1] and max(r["v"] for r in t) == 16.0
    _same(rule(_rows(t), 1e-6, 8, True)[1], t)


def test_non_finite_costs_are_rejected_rows_and_the_loop_recovers(rule):
    t = _balm_script([math.nan, math.inf, 0.7, 0.6, 0.59])
    assert [int(r["accepted"]) for r in t] == [0, 0, 1, 1, 1]
    got = rule(_rows(t), 1e-6, 5, True)[1]
    _same(got, t)
    assert [g["status"] for g in got] == [NONFINITE, NONFINITE, OK, OK, OK]


def test_a_rejected_row_stops_balm_and_not_the_pose_graph(rule):
    t = _balm_script([0.5, 0.5 * (1 + 1e-9), 0.4], rel_tol=1e-6)
    assert [int(r["accepted"]) for r in t] == [1, 0]          # the oracle left its loop after 2 of 3 rows
    _same(rule(_rows(t), 1e-6, 3, True)[1], t)
    _same(rule(_rows(t), 1e-6, 3, False)[1], t, ended=False)


def test_max_iter_ends_the_loop(rule):
    t = _balm_script([0.9, 1.0, 0.8, 0.7], max_iter=4)
    assert len(t) == 4
    _same(rule(_rows(t), 1e-6, 4, True)[1], t)


@pytest.mark.parametrize("name", ["pair", "ring64", "two laps", "cauchy", "lever"])
def test_pose_graph_cases_equal_their_oracle(rule, name):
    o = pg.options(**pgc.named(name)["opts"])
    t = pgc.oracle(name)["trace"]
    print(f"{name}: {len(t)} rows")
    _same(rule(_rows(t), o["rel_tol"], o["max_iter"], False)[1], t)


class _Scripted(pg.Graph):
    """a graph whose costs are scripted: relax() keeps its control flow, H and g are fixed"""

    def __init__(self, costs):
        c = pgc.named("pair")
        super().__init__(c["X"], c["closures"])
        self.todo, self.trial = list(costs), 1.0

    def assemble(self, x):
        return np.diag(np.arange(4.0, 16.0)), np.linspace(-0.5, 0.6, 12), self.trial

    def cost(self, x):
        if self.todo:
            self.trial = self.todo.pop(0)
        return self.trial


def test_pose_graph_reject_chain_equals_its_oracle(rule):
    """None of the shared cases rejects a step; this one does."""
    t = _Scripted(REJECT_CHAIN).relax(max_iter=8, rel_tol=1e-6)["trace"]
    assert [r["accepted"] for r in t] == [0, 0, 0, 1, 0, 1, 1, 1] and max(r["v"] for r in t) == 16.0
    _same(rule(_rows(t), 1e-6, 8, False)[1], t)


def test_flagged_rows_are_rejected_whatever_the_trial_cost(rule):
    for r2 in (0.5, 2.0, math.nan):
        done0, got = rule([(1.0, r2, 0.3, 1.0), (1.0, 0.5, 0.3, 0.0)], 1e-6, 10, True, u0=0.01, v0=2.0)
        plain = rule([(1.0, 2.0, 0.3, 0.0), (1.0, 0.5, 0.3, 0.0)], 1e-6, 10, True, u0=0.01, v0=2.0)[1]
        assert not done0
        assert got[0]["accepted"] == 0 and got[0]["status"] == FACTORIZATION and math.isnan(got[0]["q"]) and not got[0]["done"]
        # u and v move as on a plain rejection, and the next row is not evaluated again
        assert (got[1]["u"], got[1]["v"], got[1]["evaluated"]) == (plain[1]["u"], plain[1]["v"], 0) == (0.01 * 2.0, 4.0, 0)


def test_no_iterations(rule):
    assert rule([], 1e-6, 0, True)[0] and rule([], 1e-6, 0, False)[0]
    assert not rule([], 1e-6, 1, True)[0]
