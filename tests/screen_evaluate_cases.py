"""The inputs of the evaluation's tests (tests/test_screen_evaluate_cpu.py, tests/test_screen_evaluate_gpu.py): the lists of
tests/screen_components_cases.py under three partitions each, directed lists for the duplicate runs, the contended destinations, the ties
and the masks, and a reference that shares nothing with pyani_amd/screen.py: a brute force over a Python dict of pair -> greatest weight.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.

Everything expected is an integer and must be EQUAL."""
import functools

import numpy as np

from tests import screen_components_cases as cc
from tests import screen_representatives_cases as rc

NODE_ARRAYS = ("in_pairs", "in_weight", "in_min", "out_pairs", "out_weight", "out_node", "to_medoid")
CLUSTER_ARRAYS = ("size", "pairs", "weight", "min", "medoid", "near_weight", "near_cluster")
NODE_TYPES = (np.uint32, np.uint64, np.uint32, np.uint32, np.uint32, np.int32, np.uint32)
CLUSTER_TYPES = (np.uint32, np.uint64, np.uint64, np.uint32, np.int32, np.uint32, np.int32)
NONE = 0xFFFFFFFF
TOP = 2 ** 32 - 1

PARTITIONS = ("rep", "root", "random")
BRUTE_CASES = sorted(set(cc.CASES) - {"largest"})      # largest has 2^20 nodes: the brute force loops over the nodes in Python
PAIRS = [(name, part) for name in sorted(cc.CASES) for part in PARTITIONS]


def random_partition(n, seed):
    """int32[n]: every node drawn into one of about n / 16 + 1 groups, a group named by its smallest member — unrelated to any graph."""
    group = np.random.default_rng(seed).integers(0, n // 16 + 1, n)
    first = np.full(n // 16 + 1, n, dtype=np.int64)
    np.minimum.at(first, group, np.arange(n))
    return first[group].astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name, part):
    """(a, b, weight, n, label, score) of a list of the components' cases under one of the three partitions; the scores are the
    representatives' `random` kind.  Computed once, shared, read-only."""
    from pyani_amd import screen
    a, b, s, n = cc.CASES[name]()
    score = rc.scores("random", n)
    if part == "rep":
        label = screen.representatives_of_pairs(a, b, s, n, score)[0]
    elif part == "root":
        label = screen.components_of_pairs(a, b, s, n)[0]
    else:
        label = random_partition(n, n + 11)
    label = np.ascontiguousarray(label, dtype=np.int32)
    label.setflags(write=False)
    return a, b, s, n, label, score


# ---- directed lists ------------------------------------------------------------------------------------------------------------------------
def _directed(a, b, w, n, label, score):
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.uint32)
    return a, b, w, int(n), np.ascontiguousarray(label, dtype=np.int32), np.ascontiguousarray(score, dtype=np.uint64)


RUN_LENGTHS = (1, 63, 64, 65, 257, 1025)
RUN_PLACES = ("first", "last", "middle")


def duplicate_run(count, place):
    """The pair {2, 5} `count` times in alternating direction with distinct weights 10 ... 9 + count, the greatest of them placed first,
    last or in the middle of the list, between two single pairs {1, 5} and {2, 6}: n = 8, clusters {0, 1}, {2 ... 6}, {7}."""
    w = np.arange(10, 10 + count, dtype=np.int64)
    at = {"first": 0, "last": count - 1, "middle": count // 2}[place]
    w[[at, count - 1]] = w[[count - 1, at]]
    x = np.where(np.arange(count) % 2 == 0, 2, 5)
    a = np.concatenate([[1], x, [6]])
    b = np.concatenate([[5], 7 - x, [2]])
    return _directed(a, b, np.concatenate([[3], w, [4]]), 8, [0, 0, 2, 2, 2, 2, 2, 7], np.full(8, 1))


STAR_LEAVES = 1 << 16


def star(own_clusters, hub_last):
    """A star of 2^16 leaves, every weight 2^32 - 1, the hub node 0 (the low end of every pair) or node n - 1 (the high end).  One
    cluster: the hub's in_weight passes 2^32 and one destination takes everything.  own_clusters: every node its own cluster, so that
    the hub's out_* and its cluster's near_* maxima are the contended ones (every key ties in its weight: the smaller node wins)."""
    n = STAR_LEAVES + 1
    hub = n - 1 if hub_last else 0
    leaves = np.arange(STAR_LEAVES) + (0 if hub_last else 1)
    label = np.arange(n) if own_clusters else np.zeros(n)
    return _directed(np.full(STAR_LEAVES, hub), leaves, np.full(STAR_LEAVES, TOP, dtype=np.uint32), n, label, np.arange(n))


def medoid_tie(equal_scores):
    """Cluster {0, 3, 4, 5} with the pairs 3-4 (9) and 0-5 (2): nodes 3 and 4 tie in in_weight.  Equal scores: the medoid is 3, the
    smaller index; otherwise node 4 has the greater score and is the medoid.  Nodes 1, 2 are a second cluster without a pair."""
    score = [5] * 6 if equal_scores else [5, 5, 5, 6, 7, 5]
    return _directed([4, 5], [3, 0], [9, 2], 6, [0, 1, 1, 0, 0, 0], score)


def near_tie():
    """Clusters A = {0, 1}, B = {2, 3}, C = {4, 5}; A reaches B and C by pairs of weight 7 (0-2, 0-3, 1-4): near_cluster[A] is B (the
    smaller label) and out_node[0] is 2 (the smaller node); B and C reach only A."""
    return _directed([0, 3, 1], [2, 0, 4], [7, 7, 7], 6, [0, 0, 2, 2, 4, 4], [1, 2, 3, 4, 5, 6])


def zero_weights():
    """Clusters {0, 1}, {2}, {3}: the inside pair 0-1 and the outside pair 1-2 both weigh 0.  in_min[0] is 0 with in_pairs 1; out_node[1]
    is 2 with out_weight 0 — a pair of weight 0 is still a pair — while node 3 has -1."""
    return _directed([0, 1], [1, 2], [0, 0], 4, [0, 0, 2, 3], [1, 1, 1, 1])


def tiny(kind):
    if kind == "one_node":
        return _directed([], [], [], 1, [0], [9])
    if kind == "no_entries":
        return _directed([], [], None, 5, [0, 0, 2, 2, 2], [1, 2, 3, 4, 5])
    if kind == "unweighted":      # a triangle and a tail, every entry weighs 1, one pair given twice
        return _directed([0, 1, 2, 2, 1], [1, 2, 0, 3, 0], None, 5, [0, 0, 0, 3, 4], [1, 2, 3, 4, 5])
    if kind == "self_only":
        return _directed([0, 3, 3, 4], [0, 3, 3, 4], [7, 8, 9, 10], 5, [0, 0, 0, 3, 3], [5, 4, 3, 2, 1])
    raise KeyError(kind)


DIRECTED = {f"run_{c}_{p}": (lambda c=c, p=p: duplicate_run(c, p)) for c in RUN_LENGTHS for p in RUN_PLACES}
DIRECTED.update({
    "star_one_cluster": lambda: star(False, False), "star_one_cluster_hub_last": lambda: star(False, True),
    "star_own_clusters": lambda: star(True, False), "star_own_clusters_hub_last": lambda: star(True, True),
    "medoid_tie_equal_scores": lambda: medoid_tie(True), "medoid_tie_unequal_scores": lambda: medoid_tie(False),
    "near_tie": near_tie, "zero_weights": zero_weights,
    "one_node": lambda: tiny("one_node"), "no_entries": lambda: tiny("no_entries"), "unweighted": lambda: tiny("unweighted"),
    "self_only": lambda: tiny("self_only"),
})

# what the list entry refuses before it copies or replaces anything, beside cc.REFUSALS: a label array over 4 nodes and the word the
# message must hold
LABEL_REFUSALS = {"label_below": ([0, -1, 2, 2], "node 1"), "label_at_n": ([0, 0, 4, 3], "node 2"), "label_not_naming": ([0, 0, 1, 3], "node 2")}


# ---- the reference: a brute force in Python integers -------------------------------------------------------------------------------------------
def brute(a, b, weight, n, label, score):
    """(seven node arrays, seven cluster arrays) from a dict of pair -> greatest weight and plain loops."""
    pair = {}
    ws = [1] * len(a) if weight is None else weight.tolist()
    for x, y, w in zip(a.tolist(), b.tolist(), ws):
        if x != y:
            k = (min(x, y), max(x, y))
            pair[k] = max(pair.get(k, -1), w)
    lab, sc = label.tolist(), score.tolist()
    rank = {v: i for i, v in enumerate(sorted(range(n), key=lambda v: (-sc[v], v)))}
    in_pairs, in_weight, in_min, out_pairs = [0] * n, [0] * n, [NONE] * n, [0] * n
    out_best, near_best = [None] * n, [None] * n
    size, pairs, weight_c = [0] * n, [0] * n, [0] * n
    min_c = [NONE if lab[v] == v else 0 for v in range(n)]
    for (u, v), w in pair.items():
        if lab[u] == lab[v]:
            c = lab[u]
            pairs[c] += 1
            weight_c[c] += w
            min_c[c] = min(min_c[c], w)
        for p, q in ((u, v), (v, u)):
            if lab[p] == lab[q]:
                in_pairs[p] += 1
                in_weight[p] += w
                in_min[p] = min(in_min[p], w)
            else:
                out_pairs[p] += 1
                if out_best[p] is None or (w, -q) > out_best[p]:
                    out_best[p] = (w, -q)
                if near_best[lab[p]] is None or (w, -lab[q]) > near_best[lab[p]]:
                    near_best[lab[p]] = (w, -lab[q])
    best = {}
    for v in range(n):
        size[lab[v]] += 1
        key = (in_weight[v], -rank[v])
        if lab[v] not in best or key > best[lab[v]][0]:
            best[lab[v]] = (key, v)
    medoid = [best[v][1] if lab[v] == v else -1 for v in range(n)]
    to_medoid = [0] * n
    for (u, v), w in pair.items():
        if lab[u] == lab[v]:
            for p, q in ((u, v), (v, u)):
                if medoid[lab[p]] == q:
                    to_medoid[p] = w
    out_weight = [0 if x is None else x[0] for x in out_best]
    out_node = [-1 if x is None else -x[1] for x in out_best]
    near_weight = [0 if x is None else x[0] for x in near_best]
    near_cluster = [-1 if x is None else -x[1] for x in near_best]
    nodes = (in_pairs, in_weight, in_min, out_pairs, out_weight, out_node, to_medoid)
    clusters = (size, pairs, weight_c, min_c, medoid, near_weight, near_cluster)
    return (tuple(np.array(x, dtype=t) for x, t in zip(nodes, NODE_TYPES)), tuple(np.array(x, dtype=t) for x, t in zip(clusters, CLUSTER_TYPES)))


def same(got, want, what):
    """Both halves of an evaluation equal, in type, shape and every value."""
    for half, names, types in ((0, NODE_ARRAYS, NODE_TYPES), (1, CLUSTER_ARRAYS, CLUSTER_TYPES)):
        assert len(got[half]) == len(want[half]) == len(names), what
        for g, w, dtype, name in zip(got[half], want[half], types, names):
            assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


@functools.lru_cache(maxsize=None)
def statement(name, part):
    """evaluate_of_pairs of case(name, part): computed once, shared, read-only."""
    from pyani_amd import screen
    out = screen.evaluate_of_pairs(*case(name, part))
    for half in out:
        for x in half:
            x.setflags(write=False)
    return out
