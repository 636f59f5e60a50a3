"""The inputs of the linkage's tests (tests/test_screen_linkage_cpu.py, tests/test_screen_linkage_gpu.py): lists of pairs with distances
whose components have chosen sizes, and a reference that shares nothing with pyani_amd/screen.py: per component the distance matrix from
Python dicts, scipy's linkage and fcluster on it, and a plain walk for the representatives.  TEST INFRASTRUCTURE ONLY: nothing under
pyani_amd/ imports this file.

Everything expected is an integer or a double whose bits are fixed, and must be EQUAL (tests/heatmap_cases.same_bits): no tolerance."""
import functools

import numpy as np

MAX_N = 1 << 20
SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 1025)      # either side of every small limit, one past a wave, one past the workgroup's threads


def graph(sizes, seed, chords=1.0, quantum=0, spread=0.3, scramble=True):
    """(a int32[m], b int32[m], dist float64[m], n): one component per size — a chain over its members plus about chords * size random
    chords, so that `fill` cells occur inside it — under scrambled node labels (the components interleave), one direction each, in
    shuffled order.  dist: uniform in (0, spread), or with quantum q a multiple k / q, 1 <= k <= q * spread (exact in binary: ties are
    everywhere)."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    label = rng.permutation(n) if scramble else np.arange(n)
    us, vs = [], []
    at = 0
    for s in sizes:
        s = int(s)
        if s >= 2:
            u = np.arange(s - 1)
            us.append(at + u)
            vs.append(at + u + 1)
            if s >= 4:
                k = int(chords * s)
                x, y = rng.integers(0, s, k), rng.integers(0, s, k)
                keep = np.abs(x - y) > 1
                us.append(at + x[keep])
                vs.append(at + y[keep])
        at += s
    u = np.concatenate(us) if us else np.zeros(0, np.int64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.int64)
    m = len(u)
    if quantum:
        dist = rng.integers(1, max(2, int(quantum * spread)) + 1, m).astype(np.float64) / float(quantum)
    else:
        dist = rng.random(m) * spread + 1e-6
    flip = rng.random(m) < 0.5
    a, b = np.where(flip, v, u), np.where(flip, u, v)
    order = rng.permutation(m)
    return _case(label[a][order], label[b][order], dist[order], n)


def _case(a, b, dist, n):
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    for x in (a, b, dist):
        x.setflags(write=False)
    return a, b, dist, int(n)


def sizes_case():
    """Component sizes 1, 2, 3, 31, 32, 33, 63, 64, 65 and 1025 in one list."""
    return graph(SIZES, 11)


def quantised():
    """Distances that are multiples of 1 / 64 up to 8 / 64: ties everywhere.  Components of 2 ... 70 nodes."""
    return graph((2, 5, 5, 17, 33, 40, 64, 70, 1, 3), 12, chords=2.0, quantum=64, spread=0.125)


def many():
    """5003 components of 2 ... 6 nodes: the wave kernel's packing, and a last workgroup that is only partly filled (5003 is odd)."""
    rng = np.random.default_rng(13)
    return graph(np.concatenate([rng.integers(2, 7, 5000), [2, 3, 5]]), 14)


def few():
    """Seven components of 2 ... 40 nodes: the list of the batch settings (a budget of one or two components per batch)."""
    return graph((40, 2, 9, 33, 17, 1, 5, 3), 15, chords=1.5)


def largest():
    """n = 2^20 with about 10^4 entries: nearly all nodes singletons, the components small, node 2^20 - 1 among them."""
    rng = np.random.default_rng(16)
    a = rng.integers(0, MAX_N, 10_000)
    b = np.where(rng.random(10_000) < 0.7, (a + rng.integers(1, 50, 10_000)) % MAX_N, rng.integers(0, MAX_N, 10_000))
    a[0], b[0] = MAX_N - 1, 5
    a[1], b[1] = 7, 7      # ignored
    return _case(a, b, rng.random(10_000) * 0.3, MAX_N)


def star_beyond():
    """One star of 8193 nodes: one more than the linkage takes."""
    return _case(np.zeros(8192, np.int64), np.arange(1, 8193), np.full(8192, 0.01), 8193)


def duplicates():
    """The max rule: the pair (0, 1) three times in both directions with 0.02, 0.07, 0.04 -> 0.07; (1, 2) once; a self-entry; -0.0."""
    return _case([0, 1, 0, 1, 2, 3, 4], [1, 0, 1, 2, 2, 4, 3], [0.02, 0.07, 0.04, 0.03, 0.5, -0.0, 0.0], 6)


CASES = {"sizes": sizes_case, "quantised": quantised, "many": many, "few": few, "largest": largest, "duplicates": duplicates}
# (case, method, cutoff, fill, score kind): what the GPU is held to the statement on, and the statement to scipy
RUNS = [
    ("sizes", "average", 0.1, 1.0, "random"), ("sizes", "complete", 0.1, 1.0, "random"),
    ("quantised", "complete", 6.0 / 64.0, 1.0, "reversed"), ("quantised", "average", 5.0 / 64.0, 0.5, "constant"),
    ("many", "average", 0.15, 1.0, "random"), ("many", "complete", 0.15, 1.0, "unit"),
    ("few", "average", 0.12, 1.0, "reversed"), ("few", "complete", 0.12, 1.0, "index"),
    ("largest", "average", 0.2, 1.0, "random"),
    ("duplicates", "average", 0.05, 1.0, "constant"), ("duplicates", "complete", 0.0, 1.0, "reversed"),
]


def scores(kind, n):
    """uint64[n] keys: `index` (node 0 best), `reversed` (node n - 1 best: the representative is never the cluster's label unless alone),
    `random` 40-bit values, `constant` (every tie goes to the smaller index), `unit` (score_keys of 1.0 everywhere: the bits of a double)."""
    if kind == "index":
        s = np.arange(n, dtype=np.uint64)[::-1].copy()
    elif kind == "reversed":
        s = np.arange(n, dtype=np.uint64)
    elif kind == "random":
        s = np.random.default_rng(n + 7).integers(0, 1 << 40, n).astype(np.uint64)
    elif kind == "constant":
        s = np.full(n, 5, dtype=np.uint64)
    elif kind == "unit":
        s = np.ones(n, dtype=np.float64).view(np.uint64).copy()
    else:
        raise KeyError(kind)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(name, method, cutoff, fill, kind):
    """(root, cluster, rep, merges) of a run by the STATEMENT (pyani_amd.screen.linkage_of_pairs, which tests/test_screen_linkage_cpu.py
    holds to scipy): computed once, shared, read-only."""
    from pyani_amd import screen
    a, b, dist, n = CASES[name]()
    out = screen.linkage_of_pairs(a, b, dist, n, scores(kind, n), method=method, cutoff=cutoff, fill=fill)
    for x in out:
        x.setflags(write=False)
    return out


# ---- the reference: dicts, scipy, a walk ----------------------------------------------------------------------------------------------------
def components(a, b, n):
    """[members ascending] per component, in ascending order of the smallest member: a sequential union-find in Python integers."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    groups = {}
    for v in range(n):
        groups.setdefault(find(v), []).append(v)
    return [groups[r] for r in sorted(groups)]


def matrix_of(members, cells, fill):
    """The s x s matrix of a component: cells = {(u, v): the maximum distance over the entries joining u and v, u < v}."""
    s = len(members)
    D = np.full((s, s), float(fill))
    at = {v: i for i, v in enumerate(members)}
    for (u, v), d in cells.items():
        if u in at:
            D[at[u], at[v]] = D[at[v], at[u]] = d
    np.fill_diagonal(D, 0.0)
    return D


def cells_of(a, b, dist):
    cells = {}
    for x, y, d in zip(a.tolist(), b.tolist(), dist.tolist()):
        if x != y:
            key = (min(x, y), max(x, y))
            cells[key] = max(cells.get(key, 0.0), d + 0.0)
    return cells


def by_scipy(a, b, dist, n, score, method, cutoff, fill):
    """(root, cluster, rep, [Z per component of >= 2 nodes, ascending root]) with scipy doing the linkage and the cut."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    cells = cells_of(a, b, dist)
    by_comp = {}
    comps = components(a[a != b], b[a != b], n)
    where = {}
    for c, members in enumerate(comps):
        for v in members:
            where[v] = c
    for (u, v), d in cells.items():
        by_comp.setdefault(where[u], {})[(u, v)] = d
    root, cluster, rep = (np.zeros(n, dtype=np.int32) for _ in range(3))
    sc = score.tolist()
    Zs = []
    for c, members in enumerate(comps):
        root[members] = members[0]
        if len(members) == 1:
            labels = [1]
        else:
            Z = linkage(squareform(matrix_of(members, by_comp.get(c, {}), fill), checks=False), method)
            Zs.append(Z)
            labels = fcluster(Z, cutoff, "distance").tolist()
        groups = {}
        for v, lab in zip(members, labels):
            groups.setdefault(lab, []).append(v)
        for g in groups.values():
            cluster[g] = min(g)
            rep[g] = max(g, key=lambda v: (sc[v], -v))
    return root, cluster, rep, Zs


def whole_matrix_partition(a, b, dist, n, method, cutoff, fill):
    """cluster[v] = the smallest member of v's flat cluster from ONE linkage over the whole n x n matrix, the absent cells at `fill`."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    D = matrix_of(list(range(n)), cells_of(a, b, dist), fill)
    labels = fcluster(linkage(squareform(D, checks=False), method), cutoff, "distance")
    smallest = {}
    for v, lab in enumerate(labels.tolist()):
        smallest.setdefault(lab, v)
    return np.array([smallest[lab] for lab in labels.tolist()], dtype=np.int32)
