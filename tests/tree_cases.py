"""Cases and independent helpers of the neighbour-joining tests (test_tree_cpu.py, test_tree_gpu.py).

Nothing here shares code with pyani_amd.tree: `nj_reference` restates neighbour joining in pure Python over dicts keyed by node id
(no slots, no numpy arithmetic, ties decided by the order of its loops); `parse_newick` reads a Newick string back; the additive
cases come with their generating trees as networkx graphs, whose path lengths and edge cuts are computed by networkx."""
import functools
import math
import random

import networkx as nx
import numpy as np


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


# ---- the second statement -------------------------------------------------------------------------------------------------------------
def nj_reference(D):
    """(joins, lengths, last, last_lengths) as lists.  ValueError where the statement raises it."""
    n = len(D)
    if n < 3 or any(len(row) != n for row in D):
        raise ValueError("shape")
    cell = [[float(v) for v in row] for row in D]
    for i in range(n):
        if cell[i][i] != 0.0:
            raise ValueError("diagonal")
        for j in range(n):
            if not math.isfinite(cell[i][j]):
                raise ValueError("not finite")
            if np.float64(cell[i][j]).tobytes() != np.float64(cell[j][i]).tobytes():
                raise ValueError("asymmetric")
    d = {(i, j): cell[i][j] for i in range(n) for j in range(n) if i != j}
    r = {}
    for i in range(n):
        s = 0.0
        for k in range(n):
            s = s + cell[i][k]
        if not math.isfinite(s):
            raise ValueError("row sum")
        r[i] = s
    live = list(range(n))      # ascending ids: new nodes carry the largest
    joins, lengths = [], []
    m = n
    while m > 3:
        best = None
        for x in range(m):
            i = live[x]
            for y in range(x + 1, m):
                j = live[y]
                q = (m - 2) * d[i, j] - (r[i] + r[j])
                if not math.isfinite(q):
                    raise ValueError("criterion")
                if best is None or q < best[0]:      # pairs come in ascending (i, j): the first of equals is the smallest
                    best = (q, i, j)
        _, a, b = best
        dab = d[a, b]
        la = dab / 2 + (r[a] - r[b]) / (2 * (m - 2))
        u = n + len(joins)
        joins.append((a, b))
        lengths.append((la, dab - la))
        rest = [k for k in live if k != a and k != b]
        for k in rest:
            duk = ((d[a, k] + d[b, k]) - dab) / 2
            r[k] = ((r[k] - d[k, a]) - d[k, b]) + duk
            d[u, k] = d[k, u] = duk
        r[u] = ((r[a] + r[b]) - m * dab) / 2
        live = rest + [u]
        m -= 1
        if not all(math.isfinite(r[k]) for k in live):
            raise ValueError("row sum")
    x, y, z = live
    last_lengths = [((d[x, y] + d[x, z]) - d[y, z]) / 2, ((d[x, y] + d[y, z]) - d[x, z]) / 2, ((d[x, z] + d[y, z]) - d[x, y]) / 2]
    return joins, lengths, [x, y, z], last_lengths


def equals_reference(tree, ref) -> bool:
    joins, lengths, last, last_lengths = ref
    return (np.asarray(tree.joins).reshape(-1, 2).tolist() == [list(j) for j in joins] and np.asarray(tree.last).tolist() == list(last)
            and same_bits(np.asarray(tree.lengths).reshape(-1, 2), np.array(lengths, dtype=np.float64).reshape(-1, 2))
            and same_bits(tree.last_lengths, np.array(last_lengths, dtype=np.float64)))


def same_tree(a, b) -> bool:
    """Two results of the tree calls: integers equal, doubles bit for bit."""
    return (np.array_equal(np.asarray(a[0]).reshape(-1, 2), np.asarray(b[0]).reshape(-1, 2)) and same_bits(np.asarray(a[1]).reshape(-1, 2), np.asarray(b[1]).reshape(-1, 2))
            and np.array_equal(a[2], b[2]) and same_bits(a[3], b[3]))


def tree_arrays(tree):
    return tree.joins, tree.lengths, tree.last, tree.last_lengths


# ---- Newick, read back ----------------------------------------------------------------------------------------------------------------
def parse_newick(text):
    """(edges, root): edges are (child, parent, length); a leaf is its label (str, unquoted), an inner node an int in closing order."""
    pos, stack, edges, counter, root = 0, [], [], 0, None

    def read_length(pos):
        if text[pos] != ":":
            return None, pos
        end = pos + 1
        while text[end] not in ",);":
            end += 1
        return float(text[pos + 1:end]), end

    while True:
        c = text[pos]
        if c == "(":
            stack.append([])
            pos += 1
        elif c == ",":
            pos += 1
        elif c == ")":
            me, counter = counter, counter + 1
            for child, length in stack.pop():
                edges.append((child, me, length))
            length, pos = read_length(pos + 1)
            if stack:
                stack[-1].append((me, length))
            else:
                root = me
        elif c == ";":
            assert pos == len(text) - 1 and not stack
            return edges, root
        else:
            if c == "'":
                end, label = pos + 1, []
                while True:
                    if text[end] == "'":
                        if text[end + 1:end + 2] == "'":
                            label.append("'")
                            end += 2
                            continue
                        break
                    label.append(text[end])
                    end += 1
                label, pos = "".join(label), end + 1
            else:
                end = pos
                while text[end] not in ":,);":
                    end += 1
                label, pos = text[pos:end], end
            length, pos = read_length(pos)
            stack[-1].append((label, length))


def canonical_edges(edges, leaf_index):
    """A tree's edges with every node named by (smallest leaf below it, leaves below it) and the length by its bits.  Nodes that share
    their smallest leaf are nested, so the name is unique.  edges: children before parents; leaf_index: a leaf -> its number."""
    name = {}
    below = {}
    out = set()
    for child, parent, length in edges:
        if child not in name:
            k = leaf_index(child)
            name[child] = (k, 1)
        lo, size = name[child]
        plo, psize = below.get(parent, (lo, 0))
        below[parent] = (min(lo, plo), psize + size)
        name[parent] = below[parent]
    for child, parent, length in edges:
        out.add((name[child], name[parent], np.float64(length).tobytes()))
    return out


def tree_edges(tree):
    child, parent, length = tree.edges()
    return list(zip(child.tolist(), parent.tolist(), length.tolist()))


def newick_matches(tree, text, labels=None) -> bool:
    """The string read back gives the tree's edges, bit for bit."""
    labels = [str(i) for i in range(tree.n)] if labels is None else [str(v) for v in labels]
    number = {lab: i for i, lab in enumerate(labels)}
    assert len(number) == tree.n
    edges, _ = parse_newick(text)
    n = tree.n
    got = canonical_edges(edges, lambda leaf: number[leaf] if isinstance(leaf, str) else None)
    want = canonical_edges(tree_edges(tree), lambda leaf: leaf if leaf < n else None)
    return got == want


# ---- additive matrices and the trees that made them -------------------------------------------------------------------------------
def _lengths(g, rng, zero_inner=False):
    for a, b in g.edges:
        inner = g.degree[a] > 1 and g.degree[b] > 1
        g.edges[a, b]["w"] = 0.0 if (zero_inner and inner) else rng.randint(1, 64) / 64      # k / 64: every sum and half is exact


def random_tree(n, seed, caterpillar=False, zero_inner=False):
    """An unrooted binary tree on leaves 0 ... n - 1 (inner nodes n ...): every new leaf splits a random edge (caterpillar: the edge
    of the previous leaf)."""
    rng = random.Random(seed)
    g = nx.Graph()
    inner = n
    g.add_edges_from([(0, inner), (1, inner), (2, inner)])
    for leaf in range(3, n):
        a, b = (leaf - 1, next(iter(g[leaf - 1]))) if caterpillar else rng.choice(sorted(g.edges))
        inner += 1
        g.remove_edge(a, b)
        g.add_edges_from([(a, inner), (b, inner), (leaf, inner)])
    _lengths(g, rng, zero_inner)
    return g


def balanced_tree(n, seed):
    """Leaves paired level by level; the last two subtrees are joined by one edge, so no node has degree 2."""
    rng = random.Random(seed)
    g = nx.Graph()
    level, inner = list(range(n)), n
    while len(level) > 3:
        nxt = []
        for k in range(0, len(level) - 1, 2):
            g.add_edges_from([(level[k], inner), (level[k + 1], inner)])
            nxt.append(inner)
            inner += 1
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    if len(level) == 3:
        g.add_edges_from([(v, inner) for v in level])
    else:
        g.add_edge(level[0], level[1])
    _lengths(g, rng)
    return g


def tree_matrix(g, n):
    dist = dict(nx.all_pairs_dijkstra_path_length(g, weight="w"))
    return np.array([[dist[i][j] for j in range(n)] for i in range(n)], dtype=np.float64)


def graph_splits(g, n):
    """{leaves on the side without leaf 0: length} of every edge, by cutting it."""
    out = {}
    for a, b in list(g.edges):
        w = g.edges[a, b]["w"]
        g.remove_edge(a, b)
        side = nx.node_connected_component(g, a)
        if 0 in side:
            side = nx.node_connected_component(g, b)
        g.add_edge(a, b, w=w)
        out[frozenset(v for v in side if v < n)] = w
    return out


ADDITIVE = {      # name -> (n, maker); every matrix is exactly the tree's
    "add4": (4, lambda: random_tree(4, 4)), "add5": (5, lambda: random_tree(5, 5)), "add8": (8, lambda: random_tree(8, 8)),
    "add33": (33, lambda: random_tree(33, 33)), "add65": (65, lambda: random_tree(65, 65)), "add130": (130, lambda: random_tree(130, 130)),
    "cat20": (20, lambda: random_tree(20, 20, caterpillar=True)), "bal32": (32, lambda: balanced_tree(32, 32)), "bal11": (11, lambda: balanced_tree(11, 11)),
}
STAR = "star12"      # zero-length inner edges: every criterion ties, only the path lengths are fixed


@functools.lru_cache(maxsize=None)
def additive(name):
    """(graph, matrix) of an additive case."""
    if name == STAR:
        g = random_tree(12, 12, zero_inner=True)
        return g, tree_matrix(g, 12)
    n, make = ADDITIVE[name]
    g = make()
    return g, tree_matrix(g, n)


# ---- the other matrices -----------------------------------------------------------------------------------------------------------------
def _symmetric(x):
    x = np.triu(x, 1)
    return x + x.T


def random_matrix(n, seed, scale=1.0):
    return _symmetric(np.random.default_rng(seed).uniform(0.05, 1.0, (n, n)) * scale)


def integer_matrix(n, seed, top=4):
    return _symmetric(np.random.default_rng(seed).integers(1, top + 1, (n, n)).astype(np.float64))


def duplicate_matrix(n, seed):
    """Points on a line, most of them several times: zero distances and equal rows."""
    x = np.random.default_rng(seed).integers(0, max(n // 3, 2), n).astype(np.float64) / 8
    return np.abs(x[:, None] - x[None, :])


def equal_matrix(n):
    return np.ones((n, n)) - np.eye(n)


def identity_like(n, seed):
    """1 - identity for identities 0.70 ... 1.00 given to two decimals, as a table of ANI values is."""
    ident = np.round(np.random.default_rng(seed).uniform(0.70, 1.0, (n, n)), 2)
    return _symmetric(1.0 - ident)


PLAIN = {
    "n3": lambda: random_matrix(3, 3), "n4": lambda: random_matrix(4, 4), "n5": lambda: random_matrix(5, 5),
    "rand63": lambda: random_matrix(63, 63), "rand64": lambda: random_matrix(64, 64), "rand65": lambda: random_matrix(65, 65),
    "rand127": lambda: random_matrix(127, 127), "rand129": lambda: random_matrix(129, 129),
    "int4": lambda: integer_matrix(4, 1), "int33": lambda: integer_matrix(33, 2), "int66": lambda: integer_matrix(66, 3, top=3),
    "dup21": lambda: duplicate_matrix(21, 4), "dup70": lambda: duplicate_matrix(70, 5),
    "equal3": lambda: equal_matrix(3), "equal4": lambda: equal_matrix(4), "equal17": lambda: equal_matrix(17), "equal65": lambda: equal_matrix(65),
    "ident70": lambda: identity_like(70, 6), "big40": lambda: random_matrix(40, 7, scale=1.0e6),
}
SMALL = sorted(PLAIN) + sorted(ADDITIVE) + [STAR]      # every case of n <= 130: the two statements are compared on all of them
LARGE = {"rand700": lambda: random_matrix(700, 700), "ident257": lambda: identity_like(257, 8)}      # the device only: the statement takes seconds


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name in PLAIN:
        return PLAIN[name]()
    if name in LARGE:
        return LARGE[name]()
    return additive(name)[1]


@functools.lru_cache(maxsize=None)
def statement(name):
    """The statement's tree of a case, computed once and shared (nobody changes it)."""
    from pyani_amd import tree
    return tree.nj_of_matrix(matrix(name))


def bad_inputs():
    """name -> matrix: each is a ValueError of the statement (and a refusal of the device where it has n >= 3)."""
    ok = random_matrix(6, 9)
    asym = ok.copy()
    asym[1, 4] = np.nextafter(asym[1, 4], 2.0)
    signed = ok.copy()
    signed[2, 3], signed[3, 2] = 0.0, -0.0
    diag = ok.copy()
    diag[3, 3] = 1e-300
    nan = ok.copy()
    nan[0, 5] = nan[5, 0] = np.nan
    inf = ok.copy()
    inf[2, 1] = inf[1, 2] = np.inf
    overflow = equal_matrix(4) * 1.5e308      # every row sum overflows
    late = equal_matrix(5) * 4.0e307          # the row sums hold, the criterion 3 d - (r + r) does not
    # found by search: the cells, the row sums and every criterion of the first step are finite; a row sum overflows when it is updated
    rng = np.random.default_rng(160)
    k = int(rng.integers(5, 9))
    later = _symmetric(rng.uniform(-1, 1, (k, k)) * rng.choice([1e305, 3e307, 1e308, 1.7e308], (k, k)))
    return {"overflow_later": later, "asymmetric": asym, "signed_zero": signed, "diagonal": diag, "nan": nan, "inf": inf, "overflow": overflow, "overflow_q": late}
