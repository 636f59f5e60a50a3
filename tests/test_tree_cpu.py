"""CPU: the neighbour-joining statement (pyani_amd.tree.nj_of_matrix) and the host pieces round it.

The statement equals a second, independent restatement (tests/tree_cases.py: pure Python over dicts) on every case of n <= 130:
joins equal, lengths bit for bit.  On additive matrices (branch lengths k / 64, so every operation is exact) its splits with their
lengths EQUAL the generating tree's, computed with networkx, and its path lengths equal the matrix; on a star with zero-length inner
edges, where every criterion ties, only the path lengths are held.  Bad inputs raise ValueError.  Newick strings are read back by
the helper's parser to the same edges, bit for bit; linkage_to_newick is held to scipy's to_tree; distances_of and run_tree (the
device replaced by the statement) are checked mode by mode and file by file."""
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import tree_cases as tc

ROOT = Path(__file__).resolve().parent.parent


class StatementEngine:
    """Stands where an Engine would: tree_nj is the statement."""

    def tree_nj(self, d):
        from pyani_amd import tree
        return tc.tree_arrays(tree.nj_of_matrix(d))


# ---- the statement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.SMALL)
def test_statement_equals_the_restatement(name):
    tree = tc.statement(name)
    D = tc.matrix(name)
    n = len(D)
    assert tree.n == n and tree.joins.shape == (n - 3, 2) and tree.lengths.shape == (n - 3, 2) and len(tree.last) == 3
    assert tc.equals_reference(tree, tc.nj_reference(D.tolist()))
    # the ids are what the contract says: join t makes node n + t, every node is joined once
    child, parent, _ = tree.edges()
    assert sorted(child.tolist()) == list(range(2 * n - 3)) and parent[:2 * (n - 3)].tolist() == np.repeat(np.arange(n, 2 * n - 3), 2).tolist()
    assert (tree.joins[:, 0] < tree.joins[:, 1]).all() and list(tree.last) == sorted(tree.last)


@pytest.mark.parametrize("name", sorted(tc.ADDITIVE))
def test_additive_matrices_give_their_tree_back(name):
    g, D = tc.additive(name)
    tree = tc.statement(name)
    assert tree.splits() == tc.graph_splits(g, tree.n)
    assert tc.same_bits(tree.patristic(), D)


def test_star_with_zero_inner_edges_keeps_the_path_lengths():
    _, D = tc.additive(tc.STAR)
    assert tc.same_bits(tc.statement(tc.STAR).patristic(), D)


def test_ties_go_to_the_smallest_ids():
    tree = tc.statement("equal17")      # every criterion is equal at every step
    assert tree.joins[0].tolist() == [0, 1] and tree.joins[1].tolist() == [2, 3]
    three = tc.statement("equal3")
    assert three.joins.shape == (0, 2) and three.last.tolist() == [0, 1, 2] and three.last_lengths.tolist() == [0.5, 0.5, 0.5]
    four = tc.statement("equal4")
    assert four.joins.tolist() == [[0, 1]] and four.last.tolist() == [2, 3, 4]


def test_negative_lengths_are_kept():
    D = np.array([[0, 1, 9, 9], [1, 0, 2, 9], [9, 2, 0, 9], [9, 9, 9, 0]], dtype=np.float64)
    from pyani_amd import tree
    t = tree.nj_of_matrix(D)
    assert tc.equals_reference(t, tc.nj_reference(D.tolist()))
    assert min(t.lengths.min(), t.last_lengths.min()) < 0


@pytest.mark.parametrize("name", sorted(tc.bad_inputs()))
def test_bad_inputs_raise(name):
    from pyani_amd import tree
    with pytest.raises(ValueError):
        tree.nj_of_matrix(tc.bad_inputs()[name])
    with pytest.raises(ValueError):
        tc.nj_reference(tc.bad_inputs()[name].tolist())


def test_too_small_and_not_square_raise():
    from pyani_amd import tree
    for bad in (np.zeros((2, 2)), np.zeros((1, 1)), np.zeros((0, 0)), np.zeros((3, 4)), np.zeros(5)):
        with pytest.raises(ValueError):
            tree.nj_of_matrix(bad)
    with pytest.raises(ValueError):
        tree.neighbor_joining(np.zeros((1, 1)), engine=StatementEngine())


# ---- host pieces ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n3", "n4", "rand65", "int33", "add33", "big40"])
def test_newick_reads_back_bit_for_bit(name):
    tree = tc.statement(name)
    text = tree.newick()
    assert text.endswith(");") and tc.newick_matches(tree, text)


def test_newick_of_a_caterpillar_of_3000_leaves():
    """Built by hand, not joined: the string is as deep as the tree is long, and neither side may recurse."""
    from pyani_amd import tree
    n = 3000
    rng = np.random.default_rng(1)
    joins = np.array([[0, 1]] + [[t + 1, n + t - 1] for t in range(1, n - 3)], dtype=np.int32)
    t = tree.Tree(n, joins, rng.uniform(-1, 1, (n - 3, 2)), np.array([n - 2, n - 1, 2 * n - 4], dtype=np.int32), rng.uniform(0, 1e-9, 3))
    text = t.newick()
    assert text.count("(") == n - 2 and tc.newick_matches(t, text)


def test_labels_are_quoted_where_newick_needs_it():
    tree = tc.statement("n5")
    labels = ["plain_name", "with space", "O'Neil", "a:b(c)", "semi;colon,comma"]
    text = tree.newick(labels)
    assert "'with space'" in text and "'O''Neil'" in text and "'a:b(c)'" in text and "'semi;colon,comma'" in text and "'plain_name'" not in text
    assert tc.newick_matches(tree, text, labels)
    with pytest.raises(ValueError):
        tree.newick(labels[:4])


def test_two_nodes_are_one_edge():
    from pyani_amd import tree
    t = tree.neighbor_joining(np.array([[0.0, 0.25], [0.25, 0.0]]), engine=None)      # made on the host: no engine is asked
    assert t.n == 2 and t.edges()[0].tolist() == [0] and t.edges()[1].tolist() == [1] and t.edges()[2].tolist() == [0.25]
    assert t.newick(["a", "b"]) == "(a:0.25,b:0.0);" and t.splits() == {frozenset([1]): 0.25}
    assert t.patristic().tolist() == [[0.0, 0.25], [0.25, 0.0]]


def _scipy_edges(Z):
    from scipy.cluster.hierarchy import to_tree
    root, nodes = to_tree(Z, rd=True)
    edges = []
    for node in nodes:
        if not node.is_leaf():
            for kid in (node.left, node.right):
                edges.append((kid.id, node.id, node.dist - kid.dist))
    return edges


@pytest.mark.parametrize("case", ["ties", "chain", "random"])
def test_linkage_to_newick_against_scipy(case):
    from scipy.cluster.hierarchy import linkage
    from pyani_amd import tree
    rng = np.random.default_rng(3)
    x = {"ties": np.repeat(np.arange(6.0), 3)[:, None], "chain": np.cumsum(np.arange(1.0, 41.0))[:, None], "random": rng.normal(size=(37, 5))}[case]
    for method in ("complete", "average", "single"):
        Z = linkage(x, method=method)
        n = len(Z) + 1
        labels = [f"g{i}" for i in range(n)]
        got, _ = tc.parse_newick(tree.linkage_to_newick(Z, labels))
        got = tc.canonical_edges(got, lambda leaf: int(leaf[1:]) if isinstance(leaf, str) else None)
        want = tc.canonical_edges(sorted(_scipy_edges(Z), key=lambda e: e[1]), lambda leaf: leaf if leaf < n else None)
        assert got == want
    assert tree.linkage_to_newick(np.zeros((0, 4)), ["only"]) == "only;"


def test_distances_of_every_mode():
    from pyani_amd import tree
    x = np.array([[1.0, 0.9, 0.7], [0.8, 1.0, 0.6], [0.7, 0.5, 1.0]])
    frame = pd.DataFrame(x, index=["a", "b", "c"], columns=["a", "b", "c"])
    d = 1.0 - x
    for sym, want in (("mean", (d + d.T) / 2), ("min", np.minimum(d, d.T)), ("max", np.maximum(d, d.T))):
        np.fill_diagonal(want, 0.0)
        got = tree.distances_of(frame, kind="identity", symmetrize=sym)
        assert tc.same_bits(got, want) and tc.same_bits(got, got.T) and got.flags.c_contiguous
        assert tc.same_bits(tree.distances_of(d, kind="distance", symmetrize=sym), want)
    forced = tree.distances_of(x + 5.0)      # the diagonal is forced
    assert np.diagonal(forced).tolist() == [0.0, 0.0, 0.0] and forced[0, 1] == forced[1, 0] == ((0.9 + 5.0) + (0.8 + 5.0)) / 2
    holes = frame.copy()
    holes.iloc[1, 2] = np.nan
    holes.iloc[0, 0] = np.nan      # the diagonal is forced to 0 whatever it holds
    with pytest.raises(ValueError, match=r"\(b, c\)"):
        tree.distances_of(holes, kind="identity")
    filled = tree.distances_of(holes, kind="identity", symmetrize="max", fill=1.0)
    assert filled[1, 2] == filled[2, 1] == 1.0 and filled[0, 0] == 0.0
    with pytest.raises(ValueError, match=r"\(1, 2\)"):
        tree.distances_of(holes.to_numpy())
    for bad in (dict(kind="similarity"), dict(symmetrize="median")):
        with pytest.raises(ValueError):
            tree.distances_of(frame, **bad)
    with pytest.raises(ValueError):
        tree.distances_of(np.zeros((2, 3)))


def test_neighbor_joining_refuses_what_the_device_refuses():
    from pyani_amd import tree
    inf = tc.bad_inputs()["inf"]
    with pytest.raises(ValueError):
        tree.neighbor_joining(inf, engine=StatementEngine())
    with pytest.raises(ValueError):
        tree.neighbor_joining(tc.bad_inputs()["overflow"], engine=StatementEngine())


def test_run_tree_files(tmp_path):
    from pyani_amd import tree
    D = tc.matrix("add8")
    names = [f"GCF_{i:03d}.1 strain {i}" if i % 2 else f"GCA_{i:03d}" for i in range(8)]
    frame = pd.DataFrame(1.0 - D / 4, index=names, columns=names)      # identities; 1 - (1 - D / 4) is exact for multiples of 1 / 256
    tab = tmp_path / "ANIm_percentage_identity.tab"
    frame.to_csv(tab, index=True, sep="\t")
    run = tree.run_tree(tab, tmp_path / "out", kind="identity", engine=StatementEngine())
    want = tree.nj_of_matrix(D / 4)
    assert tc.same_tree(tc.tree_arrays(run.tree), tc.tree_arrays(want)) and run.tree.labels == names
    assert run.newick_path == tmp_path / "out" / "tree_output" / "ANIm_percentage_identity_nj.nwk"
    assert run.edges_path == tmp_path / "out" / "tree_output" / "ANIm_percentage_identity_nj_edges.tab"
    text = run.newick_path.read_text()
    assert text == run.newick + "\n" and tc.newick_matches(want, text.strip(), names)
    edges = pd.read_csv(run.edges_path, sep="\t", float_precision="round_trip", keep_default_na=False)
    child, parent, length = want.edges()
    assert edges["child"].tolist() == child.tolist() and edges["parent"].tolist() == parent.tolist()
    assert tc.same_bits(edges["length"].to_numpy(), length)
    assert edges["label"].tolist() == [names[c] if c < 8 else "" for c in child.tolist()]
    # a frame, other labels, nothing written
    quiet = tree.run_tree(frame, kind="identity", labels=list("abcdefgh"), write_output=False, engine=StatementEngine())
    assert quiet.newick_path is None and quiet.edges_path is None and tc.newick_matches(want, quiet.newick, list("abcdefgh"))
    with pytest.raises(ValueError):
        tree.run_tree(frame, kind="identity", engine=StatementEngine())      # files wanted, no directory named


# ---- the C ABI, as far as it shows without a device -----------------------------------------------------------------------------------
def test_tree_symbols_in_header_binding_and_library():
    from pyani_amd import _lib, build
    build.build_gpu()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    for sym, arity in (("pg_tree_nj", 7), ("pg_tree_nj_set", 2), ("pg_tree_nj_last", 3)):
        m = re.search(rf"\b{sym}\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[sym][1]) and hasattr(lib, sym), sym
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    for name in ("tree_nj", "tree_nj_set", "tree_nj_last"):
        assert callable(getattr(Engine, name)) and callable(getattr(MultiEngine, name))
