"""Match sets for the device track builder (include/lvba_hip.h "feature tracks on the device") and what the host
mirror -- pipeline.match_graph / match_components / bfs_order, the specification -- makes of them.  Fixed seed; no test lives
here.  A case is dict(n_keypoints, keypoints: float32 [n_i, 2] per image, pairs: [(a, b)], matches: int32 [m, 2] per pair)."""
import functools
import importlib

import numpy as np

THRESHOLDS = (1, 2, 3, 5)
NAMES = ("four_views", "random", "hub", "chain", "giant", "thresholds", "no_images", "one_image", "no_pairs", "empty_pairs", "all_skipped")
EVERY_ATTEMPT = ("random", "hub", "thresholds")          # the cases whose every attempt of every component is walked
CHAIN_ATTEMPTS = (0, 1, 150, 299)
HUB_FAN = 150                                            # neighbours of the hub: 19 batches of 8 lanes, two and a part of 64 lanes


def _case(n_keypoints, pairs, matches, seed):
    rng = np.random.default_rng(seed)
    kps = [rng.uniform(0, 640, (int(n), 2)).astype(np.float32) for n in n_keypoints]
    return dict(n_keypoints=[int(n) for n in n_keypoints], keypoints=kps, pairs=[(int(a), int(b)) for a, b in pairs],
                matches=[np.asarray(m, np.int32).reshape(-1, 2) for m in matches])


def _four_views():
    """(a) the planted matches of the four views of tests/match_cases.py"""
    mc = importlib.import_module("match_cases")
    g = mc.guided()
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    return _case([len(k) for k in g["keypoints"][:4]], pairs, [sorted(mc.planted_matches(g, a, b)) for a, b in pairs], 1)


def _random():
    """(b) 7 images of 0 - 40 key points, one of them empty; the pairs in shuffled order, some as (hi, lo), one listed twice with
    overlapping matches (duplicate neighbours), negative and too large indices among the matches"""
    rng = np.random.default_rng(20)
    n = [23, 40, 0, 17, 31, 8, 36]
    pairs, matches = [], []
    for a in range(7):
        for b in range(a + 1, 7):
            m = np.stack([rng.integers(0, max(n[a], 1), 7), rng.integers(0, max(n[b], 1), 7)], 1)
            if (a + b) % 3 == 0:
                m[1] = (-1, 0)
                m[4] = (0, n[b])                           # one past the last key point
            if (a + b) % 4 == 1:
                m[2] = (n[a] + 5, -3)
            if a % 2:
                a2, b2, m = b, a, m[:, ::-1]               # given as (hi, lo)
            else:
                a2, b2 = a, b
            pairs.append((a2, b2)); matches.append(m)
    twin = pairs.index((0, 4))
    pairs.append((4, 0)); matches.append(np.vstack([matches[twin][2:6, ::-1], [[3, 3], [30, 22]]]))   # overlaps the first listing
    order = rng.permutation(len(pairs))
    return _case(n, [pairs[k] for k in order], [matches[k] for k in order], 2)


def _hub():
    """(c) key point 1 of image 0 is matched by HUB_FAN key points of image 1, which fan out to images 2 - 4.  The hub's neighbour
    list crosses the batch of the BFS many times, at 8 lanes and at 64.  Planted duplicates, by their places in the list: (1, 42)
    at 43 and 45 and (1, 133) at 137 and 140 (two lanes of one batch of 8 hold the same unseen neighbour), (1, 5) at 5 and 20 and
    (1, 70) at 72 and 81 (one batch of 64, two batches of 8: already stamped in the second), (1, 10) at 10 and 102 (two batches
    of 64).  HUB_DUPLICATES has the places; the tests check them."""
    hub = [(1, k) for k in range(HUB_FAN)]
    for at, k in ((20, 5), (100, 10), (80, 70), (45, 42), (140, 133)):
        hub.insert(at, (1, k))
    pairs, matches = [(0, 1)], [hub]
    for t in (2, 3, 4):
        fan = [(k, k // 3) for k in range(HUB_FAN) if k % 3 == t - 2]
        fan += [(k, (k // 3 + 7) % 50) for k in range(0, HUB_FAN, 11) if k % 3 == t - 2]      # two key points of image 1 share one
        pairs.append((1, t)); matches.append(fan)
    pairs.append((3, 2)); matches.append([(k, k) for k in range(0, 50, 5)])
    return _case([3, HUB_FAN + 10, 60, 60, 60], pairs, matches, 3)


HUB_DUPLICATES = {5: (5, 20), 10: (10, 102), 42: (43, 45), 70: (72, 81), 133: (137, 140)}


def _chain():
    """(d) 300 nodes over 300 images in one path whose node ids descend from one end to the other: the smallest label travels the
    whole length"""
    rng = np.random.default_rng(23)
    pairs = [(i + 1, i) for i in range(299)]
    order = rng.permutation(len(pairs))
    return _case([1] * 300, [pairs[k] for k in order], [[(0, 0)]] * 299, 4)


def _giant():
    """(e) one component of 5 000 nodes (a random tree over 125 key points of each of 40 images) beside 1 000 tracks of 3 - 6 views"""
    rng = np.random.default_rng(24)
    M, per, n_tracks = 40, 125, 1000
    by_pair = {}
    img = rng.integers(0, M, M * per)
    img[:M] = np.arange(M)
    count = np.zeros(M, np.int64)
    node = []
    for i in img:                                          # node t = (image, next free key point of it)
        node.append((int(i), int(count[i]))); count[i] += 1
    for t in range(1, len(node)):
        while True:
            s = int(rng.integers(0, t))
            if node[s][0] != node[t][0]:
                break
        (a, ka), (b, kb) = sorted([node[s], node[t]])
        by_pair.setdefault((a, b), []).append((ka, kb))
    base = int(count.max())
    for t in range(n_tracks):
        views = int(rng.integers(3, 7))
        first = int(rng.integers(0, M - views + 1))
        for v in range(first, first + views - 1):
            by_pair.setdefault((v, v + 1), []).append((base + t, base + t))
    pairs = sorted(by_pair)
    return _case([base + n_tracks] * M, pairs, [by_pair[p] for p in pairs], 5)


def _thresholds():
    """(f) 6 nodes in 2 images (enough nodes, too few images), 5 nodes in 4 images, and paths of 2, 3, 4 and 5 nodes over as many
    images: for every obser_thr of THRESHOLDS a component with exactly thr nodes in exactly thr images and one with one fewer
    (a component has at least one edge, hence at least 2 nodes in 2 images)"""
    by_pair = {(0, 1): [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)]}                # a zigzag over key points 0 - 2 of images 0 and 1
    kp = 3
    for length in (2, 3, 4, 5):
        for v in range(length - 1):
            by_pair.setdefault((v, v + 1), []).append((kp, kp))
        kp += 1
    for v in range(3):                                                          # 5 nodes in 4 images: a path and a second key point
        by_pair.setdefault((v + 1, v + 2), []).append((kp, kp))
    by_pair[(1, 2)].append((kp + 1, kp))
    pairs = sorted(by_pair)
    return _case([kp + 2] * 5, pairs, [by_pair[p] for p in pairs], 6)


_BUILDERS = dict(
    four_views=_four_views, random=_random, hub=_hub, chain=_chain, giant=_giant, thresholds=_thresholds,
    no_images=lambda: _case([], [], [], 7),                                                             # (g)
    one_image=lambda: _case([5], [], [], 8),
    no_pairs=lambda: _case([4, 0, 6], [], [], 9),
    empty_pairs=lambda: _case([4, 3, 6], [(0, 1), (2, 1)], [np.zeros((0, 2)), np.zeros((0, 2))], 10),
    all_skipped=lambda: _case([4, 3, 6], [(0, 1), (2, 1), (0, 2)], [[(4, 0), (-1, 2)], [(6, 0)], [(0, -1), (9, 9)]], 11))


@functools.lru_cache(None)
def case(name):
    return _BUILDERS[name]()


def pipeline():
    return importlib.import_module("global-lvba_amd.pipeline")


@functools.lru_cache(None)
def graph(name):
    """(adj, kp_off) of the host mirror"""
    c = case(name)
    return pipeline().match_graph(c["n_keypoints"], c["pairs"], c["matches"]), np.concatenate([[0], np.cumsum(c["n_keypoints"])]).astype(np.int64)


@functools.lru_cache(None)
def expected(name, thr):
    """what lvba_trackgraph_create / _components report: dict(info, comps, comp_off, mem_img, mem_kp, comp_images, adj_off, adj)"""
    c = case(name)
    pl = pipeline()
    adj, kp_off = graph(name)
    _, comps = pl.match_components(c["n_keypoints"], c["pairs"], c["matches"], thr)
    _, every = pl.match_components(c["n_keypoints"], c["pairs"], c["matches"], 1)
    n_valid = sum(int(((m >= 0).all(1) & (m[:, 0] < c["n_keypoints"][a]) & (m[:, 1] < c["n_keypoints"][b])).sum())
                  for (a, b), m in zip(c["pairs"], c["matches"]))
    info = dict(n_nodes=sum(len(a) for a in adj), n_edges=n_valid, n_skipped=sum(len(m) for m in c["matches"]) - n_valid,
                n_components_all=len(every), n_components=len(comps), n_observations=sum(len(m) for m in comps),
                largest_component=max([len(m) for m in comps], default=0))
    flat = [ob for m in comps for ob in m]
    adj_off, flat_adj = [0], []
    for i, a in enumerate(adj):
        for k in range(c["n_keypoints"][i]):
            flat_adj += [int(kp_off[j]) + kj for j, kj in a.get(k, ())]
            adj_off.append(len(flat_adj))
    return dict(info=info, comps=comps, comp_off=np.concatenate([[0], np.cumsum([len(m) for m in comps])]).astype(np.int64),
                mem_img=np.array([i for i, _ in flat], np.int32), mem_kp=np.array([k for _, k in flat], np.int32),
                comp_images=np.array([len({i for i, _ in m}) for m in comps], np.int32),
                adj_off=np.asarray(adj_off, np.int64), adj=np.asarray(flat_adj, np.int64))


@functools.lru_cache(None)
def order_of(name, thr, c, attempt):
    return pipeline().bfs_order(graph(name)[0], expected(name, thr)["comps"][c][attempt])


def expected_orders(name, thr, attempt, comp=None):
    """(obs_off, obs_img, obs_kp) of the components `comp` (None: all) for one attempt"""
    comp = range(len(expected(name, thr)["comps"])) if comp is None else comp
    orders = [order_of(name, thr, int(c), attempt) for c in comp]
    flat = [ob for o in orders for ob in o]
    return (np.concatenate([[0], np.cumsum([len(o) for o in orders])]).astype(np.int64), np.array([i for i, _ in flat], np.int32),
            np.array([k for _, k in flat], np.int32))


def attempts_of(name, thr):
    """the attempts the tests walk for a case: every one up to the largest component where the issue asks for that"""
    sizes = [len(m) for m in expected(name, thr)["comps"]]
    if name in EVERY_ATTEMPT:
        return list(range(max(sizes, default=0)))
    if name == "chain":
        return [a for a in CHAIN_ATTEMPTS if sizes and a < max(sizes)]
    return [0] if sizes else []


def with_more_than(name, thr, attempt):
    """the components that have an attempt `attempt`"""
    return [c for c, m in enumerate(expected(name, thr)["comps"]) if len(m) > attempt]
