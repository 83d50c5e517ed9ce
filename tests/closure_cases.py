"""The shared closure-consistency cases of tests/test_closure_host.py and tests/test_gpu_closure.py, computed once per process
(DESIGN.md §10f).

Trajectories: loop_cases.laps() (three laps of 40 frames on a grid of 1 m, lap 2 on the very positions of lap 1, lap 3 1 m higher)
with headings along the path and a little roll and pitch, so that every rotation matters; the same far from the origin; and §10e's
two laps at the drifted poses (place_cases.drifted()).

A closure of group g is Z_k = X_i^-1 D_g^-1 X_j N_k: D_g a rigid world-frame discrepancy per group, N_k a small perturbation per
closure.  Within a group the cycle is N_a (seen from j_a) against N_b; across groups it is D_g^-1 D_h seen from i_a.
"""
from __future__ import annotations

import functools

import numpy as np

import closure_oracle as co
import loop_cases as lc
import place_cases as pc


def rx(a):
    return co.exp([a, 0, 0])[:9].reshape(3, 3)


def ry(a):
    return co.exp([0, a, 0])[:9].reshape(3, 3)


def rz(a):
    return co.exp([0, 0, a])[:9].reshape(3, 3)


@functools.lru_cache(maxsize=None)
def _headed(offset):
    P = lc.laps().copy()
    for f in range(len(P)):
        yaw = 0.5 * np.pi * ((f % 40) // 10) + 0.05 * np.sin(0.9 * f) + 0.02 * (f // 40)
        P[f, :9] = (rz(yaw) @ rx(0.02 * np.sin(1.3 * f)) @ ry(0.015 * np.cos(0.7 * f))).reshape(9)
        P[f, 9:] += offset
    return P


def headed(offset=(0.0, 0.0, 0.0)):
    return _headed(tuple(float(v) for v in offset)).copy()


FAR = (1000.0, -1000.0, 500.0)


def closure(X, i, j, D=co.IDENTITY, N=co.IDENTITY):
    return co.mul(co.mul(co.mul(co.inv(X[i]), co.inv(D)), X[j]), N)


def noise(rng, rot=1e-3, trans=5e-3):
    return co.rigid(rng.normal(size=3) * rot, rng.normal(size=3) * trans)


# the discrepancies of the outlier groups: far beyond the tolerances at any path length of these trajectories (L <= 240: 0.275 rad,
# 2.6 m), and as far from one another
GROUPS = [co.IDENTITY, co.rigid(t=(6.0, 0, 0)), co.rigid(t=(0, -7.0, 0)), co.rigid((0, 0, 0.6), (0, 0, 0)), co.rigid(t=(0, 0, 9.0)),
          co.rigid((0.5, 0, 0), (5.0, 5.0, 0)), co.rigid(t=(-8.0, 8.0, 0)), co.rigid((0, 0.7, 0), (0, 0, -6.0)), co.rigid(t=(12.0, 0, 3.0))]


def grouped(X, M, group_of, seed):
    """M closures lap 1 -> laps 2 and 3, closure k in group group_of(k), with a little noise each."""
    rng = np.random.default_rng(seed)
    ref, query, Z, g = [], [], [], []
    for k in range(M):
        i = (7 * k) % 40
        j = 40 + (i + 3 * (k // 40) + (40 if k % 3 == 2 else 0)) % 80
        ref.append(i); query.append(j); g.append(group_of(k))
        Z.append(closure(X, i, j, GROUPS[g[-1]], noise(rng)))
    return np.int32(ref), np.int32(query), np.array(Z).reshape(M, 12), g


def case(name, X, ref, query, Z, groups=None, **opts):
    return dict(name=name, X=np.ascontiguousarray(X), ref=np.int32(ref), query=np.int32(query), Z=np.ascontiguousarray(Z, np.float64).reshape(-1, 12),
                groups=groups, opts=co.options(**opts))


def _sizes():
    X = headed()
    out = []
    for M in (0, 1, 2, 63, 64, 65, 130):
        # every tenth closure an outlier, in groups of three or so (k // 30 + 1); the rest in group 0
        ref, query, Z, g = grouped(X, M, lambda k: 1 + (k // 30) % 8 if k % 10 == 9 else 0, seed=M)
        out.append(case(f"M = {M}", X, ref, query, Z, g))
    return out


def _clauses():
    """The pair-test clauses against the last closure (6: N = identity, (0, 40)).  Every closure is on lap 2, where t_j = t_i, and
    the perturbed one is the pair's first: its N turns about its own frame's position and shows in rot alone.
      0  rot 0.030, L 2: admitted, the rotation bound 0.037 the binding one      1  rot 0.050, L 4: rejected by rotation alone (0.039)
      2  trans 0.15, L 6: admitted (0.26)                                        3  trans 0.35, L 8: rejected by translation alone (0.28)
      4  trans 0.35, L 60: admitted by the rate term alone (0.8, trans_tol 0.2)  5  rot 0.050, L 70: admitted by the rate term alone (0.105)"""
    X = headed()
    items = [(1, co.rigid((0, 0, 0.030))), (2, co.rigid((0, 0, 0.050))), (3, co.rigid(t=(0.15, 0, 0))), (4, co.rigid(t=(0, 0.35, 0))),
             (30, co.rigid(t=(0, 0.35, 0))), (35, co.rigid((0, 0, 0.050))), (0, co.IDENTITY)]
    return case("clauses", X, [i for i, _ in items], [i + 40 for i, _ in items], [closure(X, i, i + 40, N=N) for i, N in items])


def _chain():
    """a ~ b, b ~ c, a !~ c: translation discrepancies 0, 0.6 and 1.2 trans_tol along one axis, no rate terms."""
    X = headed()
    tt = co.DEFAULTS["trans_tol"]
    items = [(5, 0.0), (6, 0.6 * tt), (7, 1.2 * tt)]
    return case("chain", X, [i for i, _ in items], [i + 40 for i, _ in items],
                [closure(X, i, i + 40, N=co.rigid(t=(d, 0, 0))) for i, d in items], rot_rate=0.0, trans_rate=0.0)


def _two_cliques():
    """Two disjoint cliques of five, interleaved, closure 0 in the one with the discrepancy: every degree is 4, the seed order is
    the index order and the tie between the two sets goes to the seed that comes first."""
    X = headed()
    ref, query, Z, g = grouped(X, 10, lambda k: 1 if k % 2 == 0 else 0, seed=77)
    return case("two cliques", X, ref, query, Z, g)


def _seed_cases():
    X = headed()
    ref, query, Z, g = grouped(X, 65, lambda k: 1 + (k // 30) % 8 if k % 10 == 9 else 0, seed=65)
    small = grouped(X, 20, lambda k: (0, 0, 1, 0, 2)[k % 5], seed=20)
    return [case("n_seeds 1", X, ref, query, Z, g, n_seeds=1),
            case("n_seeds > M", X, ref, query, Z, g, n_seeds=1000),
            case("min_set above the best", X, *small[:3], small[3], min_set=13),
            case("min_set met", X, *small[:3], small[3], min_set=12)]


def _far():
    """Positions ~1 000 m from the origin; group 1 is turned by 0.5 mrad about the world's z axis THROUGH THE ORIGIN: the angle is
    far below rot_tol, the lever arm makes it 0.7 m."""
    X = headed(FAR)
    rng = np.random.default_rng(9)
    D = [co.IDENTITY, co.rigid((0, 0, 5e-4))]
    ref, query, Z, g = [], [], [], []
    for k in range(18):
        i, grp = k % 10, 1 if k % 3 == 2 else 0
        j = 40 + i + (1 if k >= 10 else 0)
        ref.append(i); query.append(j); g.append(grp)
        Z.append(closure(X, i, j, D[grp], noise(rng)))
    return case("lever arm", X, ref, query, Z, g)


def two_lap_closures(extra=True):
    """§10e's revisits as closures at the drifted poses: (k, 12 + k) with the true relative pose and a little noise, then -- with
    `extra` -- a true measurement shifted by 2 m and a query tied to the wrong lap-A position."""
    P, X = pc.truth(), pc.drifted()
    rng = np.random.default_rng(12)
    ref, query, Z = [], [], []
    for k in range(12):
        ref.append(k); query.append(12 + k)
        Z.append(co.mul(co.mul(co.inv(P[k]), P[12 + k]), noise(rng)))
    if extra:
        shifted = co.mul(co.inv(P[3]), P[15])
        shifted[9:] += (2.0, 0.0, 0.0)
        ref.append(3); query.append(15); Z.append(shifted)
        ref.append(2); query.append(20); Z.append(co.mul(co.inv(P[8]), P[20]))      # frame 20 is at lap A's position 8, not 2
    return X, np.int32(ref), np.int32(query), np.array(Z).reshape(-1, 12)


def _two_laps():
    X, ref, query, Z = two_lap_closures()
    return case("two laps, drifted", X, ref, query, Z, [0] * 12 + [1, 2])


@functools.lru_cache(maxsize=None)
def cases():
    return _sizes() + [_clauses(), _chain(), _two_cliques()] + _seed_cases() + [_far(), _two_laps()]


def named(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def oracle(k):
    """(adjacency dict, greedy dict) of case k by the oracle."""
    c = cases()[k]
    o = c["opts"]
    adj = co.adjacency(c["X"], c["ref"], c["query"], c["Z"], **{t: o[t] for t in co.TOLS})
    return adj, co.greedy(adj["rows"], o["n_seeds"], o["min_set"])
