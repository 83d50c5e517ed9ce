"""Numpy restatement of the pairwise consistency of loop closures (include/lvba_hip.h, lvba_closure_consistency).

The cycle is written out from the definition with six compositions -- two inverses of poses and their two products for the odometry
legs, the inverse of Z_b, and the chain -- not from the prepared form the device uses.  Sets are Python integers used as bit-sets.
Also a brute-force maximum clique for small graphs.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(rot_tol=0.035, rot_rate=0.001, trans_tol=0.2, trans_rate=0.01, n_seeds=32, min_set=2)
TOLS = ("rot_tol", "rot_rate", "trans_tol", "trans_rate")


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    return o


def mul(A, B):
    """A o B of poses as 12 numbers (R row-major | t)."""
    RA, RB = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    return np.r_[(RA @ RB).reshape(9), RA @ B[9:] + A[9:]]


def inv(T):
    R = T[:9].reshape(3, 3)
    return np.r_[R.T.reshape(9), -(R.T @ T[9:])]


def exp(w):
    """Rodrigues, as a pose with zero translation."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        R = np.eye(3) + K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    return np.r_[R.reshape(9), 0.0, 0.0, 0.0]


def rigid(w=(0, 0, 0), t=(0, 0, 0)):
    T = exp(w)
    T[9:] = t
    return T


IDENTITY = rigid()


def cycle(X, ref, query, Z, a, b):
    """E_ab = Z_a (X_ja^-1 X_jb) Z_b^-1 (X_ib^-1 X_ia)"""
    leg_j = mul(inv(X[query[a]]), X[query[b]])
    leg_i = mul(inv(X[ref[b]]), X[ref[a]])
    return mul(mul(mul(Z[a], leg_j), inv(Z[b])), leg_i)


def measures(E):
    R = E[:9].reshape(3, 3)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0))), float(np.linalg.norm(E[9:]))


def path(ref, query, a, b):
    return abs(int(query[a]) - int(query[b])) + abs(int(ref[a]) - int(ref[b]))


def decide(rot, trans, L, o):
    """(consistent, margin): the margin is how far rot / trans may move before the decision changes."""
    dr = o["rot_tol"] + o["rot_rate"] * float(L) - rot
    dt = o["trans_tol"] + o["trans_rate"] * float(L) - trans
    ok = dr >= 0 and dt >= 0
    return ok, (min(dr, dt) if ok else max(-dr if dr < 0 else 0.0, -dt if dt < 0 else 0.0))


def adjacency(X, ref, query, Z, **opts):
    """dict(rows: a list of M Python integers (bit b of rows[a] is the decision), rot, trans [M, M], L [M, M], margin: the smallest
    decision margin)."""
    o = options(**opts)
    X, Z = np.asarray(X, np.float64).reshape(-1, 12), np.asarray(Z, np.float64).reshape(-1, 12)
    M = len(Z)
    rows = [1 << a for a in range(M)]
    rot, trans, L = np.zeros((M, M)), np.zeros((M, M)), np.zeros((M, M), np.int64)
    margin = np.inf
    for a in range(M):
        for b in range(a + 1, M):
            r, t = measures(cycle(X, ref, query, Z, a, b))
            l = path(ref, query, a, b)
            ok, m = decide(r, t, l, o)
            margin = min(margin, m)
            rot[a, b] = rot[b, a] = r
            trans[a, b] = trans[b, a] = t
            L[a, b] = L[b, a] = l
            if ok:
                rows[a] |= 1 << b
                rows[b] |= 1 << a
    return dict(rows=rows, rot=rot, trans=trans, L=L, margin=float(margin))


def words(rows, M):
    """The adjacency as the library lays it out: uint64 [M][ceil(M / 64)]."""
    W = (M + 63) // 64
    out = np.zeros((M, W), np.uint64)
    for a in range(M):
        for w in range(W):
            out[a, w] = (rows[a] >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def rows_of(words_):
    """The inverse of words()."""
    return [sum(int(v) << (64 * w) for w, v in enumerate(r)) for r in np.asarray(words_, np.uint64)]


def dense(rows, M):
    return np.array([[(rows[a] >> b) & 1 for b in range(M)] for a in range(M)], bool).reshape(M, M)


def bits(s):
    out = []
    while s:
        low = s & -s
        out.append(low.bit_length() - 1)
        s ^= low
    return out


def popcount(s):
    return bin(s).count("1")


def greedy(rows, n_seeds=32, min_set=2):
    """The set search of the header on adjacency rows: dict(deg, seeds, picks (per seed, in order), sets (per seed, an integer),
    best (index into seeds), keep (list of bool), n_keep)."""
    M = len(rows)
    deg = [popcount(r) - 1 for r in rows]
    seeds = sorted(range(M), key=lambda v: (-deg[v], v))[:min(n_seeds, M)]
    picks, sets = [], []
    for s in seeds:
        K, C, mine = 1 << s, rows[s] & ~(1 << s), []
        while C:
            v = min(bits(C), key=lambda u: (-popcount(rows[u] & C), u))
            mine.append(v)
            K |= 1 << v
            C = C & rows[v] & ~(1 << v)
        picks.append(mine)
        sets.append(K)
    best = min(range(len(seeds)), key=lambda k: (-popcount(sets[k]), k)) if seeds else None
    K = sets[best] if seeds and popcount(sets[best]) >= min_set else 0
    return dict(deg=deg, seeds=seeds, picks=picks, sets=sets, best=best, keep=[bool((K >> v) & 1) for v in range(M)], n_keep=popcount(K))


def is_clique(rows, K):
    return all((rows[v] & K) == K for v in bits(K))


def max_clique_size(rows):
    """Brute force (Bron-Kerbosch without pivoting) for M <= 24."""
    M = len(rows)
    assert M <= 24
    best = 0

    def grow(R, P, X):
        nonlocal best
        if not P and not X:
            best = max(best, popcount(R))
            return
        for v in bits(P):
            nb = rows[v] & ~(1 << v)
            grow(R | (1 << v), P & nb, X & nb)
            P &= ~(1 << v)
            X |= 1 << v

    grow(0, (1 << M) - 1, 0)
    return best
