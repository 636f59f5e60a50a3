"""The inputs of the components' tests (tests/test_screen_components_cpu.py, tests/test_screen_components_gpu.py) and two references that
share nothing with pyani_amd/screen.py: a union-find written here, and the roots derived from scipy.sparse.csgraph.connected_components.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.

A case is (a int32[m], b int32[m], shared uint32[m] or None, n).  What a list asks of the code is in its docstring; every list is small
enough for seconds.  Everything expected is an integer and must be EQUAL."""
import functools

import numpy as np

MAX_N = 1 << 20


def _case(a, b, shared, n):
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    s = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32)
    for x in (a, b) + (() if s is None else (s,)):
        x.setflags(write=False)
    return a, b, s, int(n)


def _both_ways(u, v, rng=None, shared=None):
    """The undirected edges (u, v) as entries in both directions, shuffled when an rng is given."""
    a, b = np.concatenate([u, v]), np.concatenate([v, u])
    s = None if shared is None else np.concatenate([shared, shared])
    if rng is not None:
        order = rng.permutation(len(a))
        a, b, s = a[order], b[order], None if s is None else s[order]
    return a, b, s


def one_node():
    """n = 1, m = 0."""
    return _case([], [], [], 1)


def self_entries():
    """n = 5 with self-entries only: five singletons, nothing counted."""
    return _case([0, 3, 3, 4], [0, 3, 3, 4], [7, 8, 9, 10], 5)


def one_direction():
    """One entry (1, 0), in one direction: node 1 owns it, node 0 is the root of both."""
    return _case([1], [0], [5], 3)


CHAIN_N = 4096


def chain(order):
    """A chain of 4096 nodes, i - (i + 1), one direction, its entries ascending, descending or shuffled: deep trees."""
    u = np.arange(CHAIN_N - 1)
    if order == "descending":
        u = u[::-1]
    elif order == "shuffled":
        u = np.random.default_rng(41).permutation(u)
    return _case(u, u + 1, (u % 7) + 1, CHAIN_N)


def chain_scrambled():
    """The chain under scrambled node labels: neighbours in the chain are far apart in the parent array."""
    rng = np.random.default_rng(42)
    label = rng.permutation(CHAIN_N)
    u = rng.permutation(CHAIN_N - 1)
    return _case(label[u], label[u + 1], None, CHAIN_N)


STAR_LEAVES = 70_000


def star():
    """A star of 70 000 leaves whose hub is node n - 1, every entry (hub, leaf): the root must become 0, every hook contends on the hub's
    tree across many workgroups, and one node owns every entry."""
    n = STAR_LEAVES + 1
    return _case(np.full(STAR_LEAVES, n - 1), np.arange(STAR_LEAVES), np.full(STAR_LEAVES, 3), n)


CLIQUE = 300


def cliques(joined, shuffled=False):
    """Two cliques of 300 in selection order (row-major, both directions: 2 x 300 x 299 entries, runs of 299 equal a across wave
    boundaries); joined: one last entry (0, 300) makes them one component, which is then not complete."""
    i, j = np.nonzero(~np.eye(CLIQUE, dtype=bool))
    a, b = np.concatenate([i, i + CLIQUE]), np.concatenate([j, j + CLIQUE])
    s = (a * 31 + b * 17) % 1000 + 1
    if joined:
        a, b, s = np.append(a, 0), np.append(b, CLIQUE), np.append(s, 5)
    if shuffled:
        order = np.random.default_rng(43).permutation(len(a))
        a, b, s = a[order], b[order], s[order]
    return _case(a, b, s, 2 * CLIQUE)


RANDOM_N, RANDOM_EDGES, RANDOM_COMPONENTS, RANDOM_LARGEST = 50_000, 30_000, 20_186, 16_106


@functools.lru_cache(maxsize=None)
def random_graph():
    """50 000 nodes, 30 000 undirected edges (the percolation edge: one large component among thousands), both directions, 1 % of the
    entries given twice, shuffled.  With seed 1 there are 20 186 components, the largest of 16 106 nodes."""
    rng = np.random.default_rng(1)
    u, v = rng.integers(0, RANDOM_N, RANDOM_EDGES), rng.integers(0, RANDOM_N, RANDOM_EDGES)
    s = rng.integers(1, 5000, RANDOM_EDGES)
    a, b, s = _both_ways(u, v, shared=s)
    twice = rng.integers(0, len(a), len(a) // 100)
    a, b, s = np.concatenate([a, a[twice]]), np.concatenate([b, b[twice]]), np.concatenate([s, s[twice]])
    order = rng.permutation(len(a))
    return _case(a[order], b[order], s[order], RANDOM_N)


def largest():
    """n = 2^20 with three entries touching node 2^20 - 1."""
    top = MAX_N - 1
    return _case([top, 5, top], [5, top, 700_000], [2, 3, 4], MAX_N)


def heavy():
    """Three entries of shared = 2^32 - 1 on one node: its weight passes 2^32."""
    return _case([2, 2, 2], [0, 1, 3], [2 ** 32 - 1] * 3, 4)


def unweighted():
    """shared=None: every entry weighs 1."""
    a, b, _, n = random_graph()
    return _case(a[:5000], b[:5000], None, n)


CASES = {
    "one_node": one_node, "self_entries": self_entries, "one_direction": one_direction,
    "chain_ascending": lambda: chain("ascending"), "chain_descending": lambda: chain("descending"), "chain_shuffled": lambda: chain("shuffled"),
    "chain_scrambled": chain_scrambled, "star": star,
    "cliques": lambda: cliques(False), "cliques_joined": lambda: cliques(True), "cliques_shuffled": lambda: cliques(False, True),
    "cliques_joined_shuffled": lambda: cliques(True, True),
    "random": random_graph, "largest": largest, "heavy": heavy, "unweighted": unweighted,
}

# n, an entry (a, b): what pg_screen_components refuses before it copies or replaces anything
REFUSALS = {"no_node": (0, None), "too_many_nodes": (MAX_N + 1, None), "index_below": (8, (-1, 3)), "index_at_n": (8, (3, 8))}


# ---- reference 1: a union-find of the tests' own ---------------------------------------------------------------------------------------------
def union_find(a, b, shared, n):
    """(root, entries, weight) by a sequential union-find with path compression, in Python integers.  Union by smaller index, so that the
    root of a tree is its smallest node."""
    parent = list(range(n))

    def find(x):
        top = x
        while parent[top] != top:
            top = parent[top]
        while parent[x] != top:
            parent[x], x = top, parent[x]
        return top
    entries, weight = [0] * n, [0] * n
    al, bl = a.tolist(), b.tolist()
    sl = [1] * len(al) if shared is None else shared.tolist()
    for x, y, s in zip(al, bl, sl):
        if x == y:
            continue
        entries[x] += 1
        weight[x] += s
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    root = np.array([find(v) for v in range(n)], dtype=np.int32)
    return root, np.array(entries, dtype=np.uint64), np.array(weight, dtype=np.uint64)


# ---- reference 2: scipy ----------------------------------------------------------------------------------------------------------------------
def scipy_roots(a, b, n):
    """(root int32[n], number of components) from scipy.sparse.csgraph.connected_components.  Its labels ascend with each component's
    smallest member (asserted here), so the smallest member of label L is the first node that carries L."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    graph = coo_matrix((np.ones(len(a), dtype=np.int8), (a.astype(np.int64), b.astype(np.int64))), shape=(n, n))
    count, label = connected_components(graph, directed=False)
    first = np.full(count, n, dtype=np.int64)
    np.minimum.at(first, label, np.arange(n))
    assert (np.diff(first) > 0).all(), "scipy's labels do not ascend with the smallest member"
    return first[label].astype(np.int32), int(count)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(root, entries, weight) of a case by the tests' union-find: computed once, shared, read-only."""
    a, b, s, n = CASES[name]()
    out = union_find(a, b, s, n)
    for x in out:
        x.setflags(write=False)
    return out
