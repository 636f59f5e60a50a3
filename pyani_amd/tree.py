"""tree — the neighbour-joining tree of a collection from its distance matrix, on the GPU.

A tree is the first thing a user builds from an ANI or Mash-like matrix.  Neighbour joining (Saitou & Nei 1987, in the form of
Studier & Keppler 1988) is n - 3 dependent steps, each an arg-min over all live pairs: O(n^3).  The device runs the steps
(pg_tree_nj, pyani_amd/csrc/pg_tree.hip); the host turns a result matrix into distances, and the joins into edges, Newick, splits
and files.  The contract is the project's usual one: the device's result EQUALS `nj_of_matrix` below, a numpy statement written to
be read, integers exactly and doubles bit for bit.

Node ids: leaves are 0 ... n - 1, join t (t = 0 ... n - 4) creates node n + t, the last node 2 n - 3 takes the three survivors.
The tree is unrooted; node 2 n - 3 is where the Newick string happens to start.  Negative branch lengths are kept as they come.

Host-only and in need of no GPU: `nj_of_matrix`, `Tree` and its methods, `distances_of`, `linkage_to_newick`.  There is no CPU
fallback for `neighbor_joining` and `run_tree`: without an engine argument they use the default engine."""
from pathlib import Path
from typing import Dict, FrozenSet, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from . import _lib

NOT_SQUARE = "a square distance matrix is needed"
TOO_FEW = "a tree needs at least two nodes"
NONFINITE = "the distance matrix, a row sum or a criterion is not finite"
ASYMMETRIC = "the distance matrix must be symmetric bit for bit"
DIAGONAL = "the diagonal of the distance matrix must be zero"
KINDS = ("identity", "distance")
SYMMETRIZE = ("mean", "min", "max")
_NEEDS_QUOTES = set(" \t\n()[]':;,")


# ---- the tree ---------------------------------------------------------------------------------------------------------------------
def _quote(label) -> str:
    """A Newick label: as it is, or in single quotes (inner ones doubled) where it holds a blank, a bracket, a quote, a colon, a
    semicolon or a comma, or is empty.  Underscores are left alone."""
    text = str(label)
    if text and not (_NEEDS_QUOTES & set(text)):
        return text
    return "'" + text.replace("'", "''") + "'"


def _newick(root: int, n_leaves: int, children: Dict[int, Sequence[Tuple[int, float]]], labels: Sequence) -> str:
    """Newick of the tree below `root`; every length as repr(float), so that a reader gets the same bits back.  Iterative: a
    caterpillar of 8192 leaves is 8190 deep."""
    out: List[str] = []
    stack: list = [(root, None)]
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            out.append(item)
            continue
        node, length = item
        suffix = "" if length is None else ":" + repr(float(length))
        if node < n_leaves:
            out.append(_quote(labels[node]) + suffix)
            continue
        out.append("(")
        stack.append(")" + suffix)
        kids = children[node]
        for k in range(len(kids) - 1, -1, -1):
            stack.append(kids[k])
            if k:
                stack.append(",")
    return "".join(out) + ";"


def _labels(labels, n: int) -> list:
    if labels is None:
        return [str(i) for i in range(n)]
    labels = list(labels)
    if len(labels) != n:
        raise ValueError(f"{n} labels are needed, not {len(labels)}")
    return labels


class Tree(NamedTuple):
    """An unrooted tree as neighbour joining records it."""
    n: int                        # leaves
    joins: np.ndarray             # (n - 3) x 2 int32: the nodes of join t, lower id first; they hang under node n + t
    lengths: np.ndarray           # (n - 3) x 2 float64: their branch lengths
    last: np.ndarray              # int32: the survivors by ascending id (three; one for n = 2), under node 2 n - 3
    last_lengths: np.ndarray      # float64: their branch lengths
    labels: Optional[list] = None # leaf labels by id, when the matrix came with some

    def edges(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(child, parent, length): the 2 n - 3 edges, joins first, in the order they were made."""
        n_joins = len(self.joins)
        child = np.concatenate([np.asarray(self.joins, dtype=np.int64).reshape(-1), np.asarray(self.last, dtype=np.int64)])
        parent = np.concatenate([np.repeat(self.n + np.arange(n_joins, dtype=np.int64), 2), np.full(len(self.last), 2 * self.n - 3, dtype=np.int64)])
        length = np.concatenate([np.asarray(self.lengths, dtype=np.float64).reshape(-1), np.asarray(self.last_lengths, dtype=np.float64)])
        return child, parent, length

    def _children(self) -> Dict[int, List[Tuple[int, float]]]:
        kids: Dict[int, List[Tuple[int, float]]] = {}
        for c, p, l in zip(*(a.tolist() for a in self.edges())):
            kids.setdefault(p, []).append((c, l))
        return kids

    def newick(self, labels=None) -> str:
        """The tree from node 2 n - 3 down: "(a:..,b:..,c:..);".  labels: one per leaf by id (default: the tree's own, else the ids).
        Two leaves give "(a:d,b:0.0);"."""
        labs = _labels(self.labels if labels is None else labels, self.n)
        if self.n == 2:
            return f"({_quote(labs[0])}:{float(self.last_lengths[0])!r},{_quote(labs[1])}:0.0);"
        return _newick(2 * self.n - 3, self.n, self._children(), labs)

    def splits(self) -> Dict[FrozenSet[int], float]:
        """Every edge as the set of leaves on its side that does NOT hold leaf 0, with the edge's length."""
        below: Dict[int, set] = {i: {i} for i in range(self.n)}
        out: Dict[FrozenSet[int], float] = {}
        everything = frozenset(range(self.n))
        for c, p, l in zip(*(a.tolist() for a in self.edges())):      # children are made before their parents
            side = frozenset(below[c])
            if p >= self.n:
                below.setdefault(p, set()).update(side)
            out[everything - side if 0 in side else side] = l
        return out

    def patristic(self) -> np.ndarray:
        """The n x n matrix of path lengths between the leaves, the lengths added from node 2 n - 3 outwards.  Memory is the square of
        the node count: for small n."""
        total = max(2 * self.n - 2, self.n)
        parent_of: Dict[int, Tuple[int, float]] = {c: (p, l) for c, p, l in zip(*(a.tolist() for a in self.edges()))}
        dist = np.zeros((total, total), dtype=np.float64)
        root = 2 * self.n - 3
        done = [root]
        for node in sorted(parent_of, reverse=True):      # a parent's id is above its children's
            if node == root:
                continue
            p, l = parent_of[node]
            row = dist[p, done] + l
            dist[node, done] = row
            dist[done, node] = row
            done.append(node)
        return dist[:self.n, :self.n].copy()


def _tree_of_two(d: float, labels=None) -> Tree:
    return Tree(2, np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.float64), np.array([0], dtype=np.int32),
                np.array([d], dtype=np.float64), labels)


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def _check_matrix(D) -> np.ndarray:
    D = np.array(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(NOT_SQUARE)
    if D.shape[0] < 3:
        raise ValueError("neighbour joining needs at least three nodes")
    if not np.isfinite(D).all():
        raise ValueError(NONFINITE)
    if not (D.view(np.int64) == D.T.copy().view(np.int64)).all():
        raise ValueError(ASYMMETRIC)
    if not (np.diagonal(D) == 0).all():
        raise ValueError(DIAGONAL)
    return D


def nj_of_matrix(D) -> Tree:
    """Neighbour joining of the finite, bit-for-bit symmetric n x n matrix D with a zero diagonal, n >= 3: THE statement the device is
    held to.  float64 throughout, every operation rounded on its own.  ValueError for anything else, and for a row sum or criterion
    that leaves the finite range.

    The live nodes sit in slots 0 ... m - 1 of the working square; `ids` names them.  Where a node is stored decides nothing: equal
    criteria go to the smallest (lower id, higher id).  The row sums are summed once, sequentially, and UPDATED after every join, not
    summed again: that is O(m) a step, and it is an order of additions that can be written down (a parallel re-summation's cannot).
    An implementation that re-sums may differ from this one at near-ties."""
    D = _check_matrix(D)
    n = len(D)
    ids = np.arange(n)
    joins, lengths = np.zeros((n - 3, 2), dtype=np.int32), np.zeros((n - 3, 2), dtype=np.float64)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.zeros(n, dtype=np.float64)
        for k in range(n):                       # sequentially, k ascending
            r = r + D[:, k]
        if not np.isfinite(r).all():
            raise ValueError(NONFINITE)
        m = n
        for t in range(n - 3):
            W, rs, pairs = D[:m, :m], r[:m], upper[:m, :m]
            Q = float(m - 2) * W - (rs[:, None] + rs[None, :])
            Qu = Q[pairs]
            if not np.isfinite(Qu).all():
                raise ValueError(NONFINITE)
            # the smallest Q; among equals (== : -0 equals +0) the smallest (lower id, higher id)
            si, sj = np.nonzero((Q == Qu.min()) & pairs)
            lo, hi = np.minimum(ids[si], ids[sj]), np.maximum(ids[si], ids[sj])
            pick = np.lexsort((hi, lo))[0]
            a, b = int(lo[pick]), int(hi[pick])
            sa, sb = (int(si[pick]), int(sj[pick])) if ids[si[pick]] == a else (int(sj[pick]), int(si[pick]))
            d = W[sa, sb]
            len_a = d / 2 + (r[sa] - r[sb]) / (2 * float(m - 2))
            joins[t], lengths[t] = (a, b), (len_a, d - len_a)
            # the new node u = n + t
            da, db = W[sa].copy(), W[sb].copy()
            du = ((da + db) - d) / 2
            ru = ((r[sa] + r[sb]) - float(m) * d) / 2
            r[:m] = ((rs - da) - db) + du
            # u takes the lower of the two slots, the last live node moves into the other (its own when it is the last)
            p, q, last = min(sa, sb), max(sa, sb), m - 1
            D[p, :m], D[:m, p], D[p, p], r[p], ids[p] = du, du, 0.0, ru, n + t
            D[q, :m], D[:m, q], D[q, q], r[q], ids[q] = D[last, :m].copy(), D[:m, last].copy(), 0.0, r[last], ids[last]
            m -= 1
            if not np.isfinite(r[:m]).all():
                raise ValueError(NONFINITE)
        x, y, z = (int(s) for s in np.argsort(ids[:3]))
        dxy, dxz, dyz = D[x, y], D[x, z], D[y, z]
        last_lengths = np.array([((dxy + dxz) - dyz) / 2, ((dxy + dyz) - dxz) / 2, ((dxz + dyz) - dxy) / 2], dtype=np.float64)
    return Tree(n, joins, lengths, ids[[x, y, z]].astype(np.int32), last_lengths)


# ---- from a result matrix to distances ----------------------------------------------------------------------------------------------
def _frame_labels(dfr) -> Optional[list]:
    return [str(v) for v in dfr.index] if isinstance(dfr, pd.DataFrame) else None


def distances_of(dfr, kind: str = "distance", symmetrize: str = "mean", fill: Optional[float] = None) -> np.ndarray:
    """The symmetric distance matrix of a square result matrix (a frame or an array), float64.
    kind: "identity" turns every cell x into 1 - x (ANI, coverage-like matrices in 0 ... 1); "distance" takes the cells as they are.
    fill: the DISTANCE a NaN cell gets (a pair without an alignment); without it a NaN cell is a ValueError naming the first pair.
    symmetrize: cells (i, j) and (j, i) become their "mean", "min" or "max" (ANIb matrices are asymmetric, ANIm's are not).
    The diagonal is forced to 0."""
    if kind not in KINDS:
        raise ValueError(f'kind must be "identity" or "distance", not {kind!r}')
    if symmetrize not in SYMMETRIZE:
        raise ValueError(f'symmetrize must be "mean", "min" or "max", not {symmetrize!r}')
    labels = _frame_labels(dfr)
    x = np.array(dfr.to_numpy() if isinstance(dfr, pd.DataFrame) else dfr, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != x.shape[1]:
        raise ValueError(NOT_SQUARE)
    if kind == "identity":
        x = 1.0 - x
    nan = np.isnan(x)
    np.fill_diagonal(nan, False)
    if nan.any():
        if fill is None:
            i, j = (int(v) for v in np.argwhere(nan)[0])
            names = (labels[i], labels[j]) if labels else (i, j)
            raise ValueError(f"no value for the pair ({names[0]}, {names[1]}); give fill= to set a distance for such pairs")
        x[nan] = float(fill)
    if symmetrize == "mean":
        with np.errstate(over="ignore"):      # a sum beyond the float range is an infinite cell: neighbor_joining refuses it
            x = (x + x.T) / 2
    else:
        x = np.minimum(x, x.T) if symmetrize == "min" else np.maximum(x, x.T)
    np.fill_diagonal(x, 0.0)
    return np.ascontiguousarray(x)


def neighbor_joining(dfr_or_array, kind: str = "distance", symmetrize: str = "mean", fill: Optional[float] = None, engine=None) -> Tree:
    """The neighbour-joining tree of a square result matrix: distances_of(...), then pg_tree_nj on the engine (default: the default
    engine).  Two nodes are one edge, made on the host; fewer are a ValueError, and so is everything the device refuses (a
    non-finite cell, an overflow).  A frame's index labels the leaves."""
    D = distances_of(dfr_or_array, kind=kind, symmetrize=symmetrize, fill=fill)
    labels = _frame_labels(dfr_or_array)
    n = len(D)
    if n < 2:
        raise ValueError(TOO_FEW)
    if not np.isfinite(D).all():
        raise ValueError(NONFINITE)
    if n == 2:
        return _tree_of_two(D[0, 1], labels)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    try:
        joins, lengths, last, last_lengths = engine.tree_nj(D)
    except _lib.PyaniGpuError as err:
        if err.code in (_lib.PG_E_NONFINITE, _lib.PG_E_ARG):
            raise ValueError(NONFINITE if err.code == _lib.PG_E_NONFINITE else str(err)) from None
        raise
    return Tree(n, joins, lengths, last, last_lengths, labels)


# ---- the dendrograms the project already computes -------------------------------------------------------------------------------------
def linkage_to_newick(Z, labels=None) -> str:
    """Newick of a linkage matrix Z (scipy's layout: the Z of graphics.heatmap_order, of graphics.merges_to_linkage over a
    ScreenLinkage's merges, or scipy's own): row t joins nodes Z[t, 0] and Z[t, 1] at height Z[t, 2] into node n + t; leaves stand at
    height 0 and a child's branch length is its parent's height minus its own.  Rooted at node 2 n - 2."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4)
    n = len(Z) + 1
    labs = _labels(labels, n)
    if n == 1:
        return _quote(labs[0]) + ";"
    height = [0.0] * n + Z[:, 2].tolist()
    children = {n + t: [(int(a), height[n + t] - height[int(a)]), (int(b), height[n + t] - height[int(b)])]
                for t, (a, b) in enumerate(Z[:, :2].tolist())}
    return _newick(2 * n - 2, n, children, labs)


# ---- a run --------------------------------------------------------------------------------------------------------------------------
class TreeRun(NamedTuple):
    tree: Tree
    newick: str
    newick_path: Optional[Path]      # None when nothing was written
    edges_path: Optional[Path]


def edges_frame(tree: Tree, labels=None) -> pd.DataFrame:
    """The edge table run_tree writes: child, parent, length, and the child's label where it is a leaf."""
    labs = _labels(tree.labels if labels is None else labels, tree.n)
    child, parent, length = tree.edges()
    return pd.DataFrame({"child": child, "parent": parent, "length": length,
                         "label": [labs[c] if c < tree.n else "" for c in child.tolist()]})


def run_tree(matrix: Union[pd.DataFrame, str, Path], outdir=None, kind: str = "distance", symmetrize: str = "mean",
             fill: Optional[float] = None, labels=None, write_output: bool = True, engine=None) -> TreeRun:
    """The tree of one result matrix, as files.  matrix: a frame, or the path of a tab-separated matrix with a header row and an index
    column (what the run drivers write as <name>.tab).  Writes <outdir>/tree_output/<stem>_nj.nwk (the Newick string and a newline)
    and <stem>_nj_edges.tab (edges_frame); stem: the file's, "matrix" for a frame.  labels: one per leaf, in place of the index."""
    stem = "matrix"
    if not isinstance(matrix, pd.DataFrame):
        stem = Path(matrix).stem
        matrix = pd.read_csv(matrix, sep="\t", index_col=0, float_precision="round_trip")
    tree = neighbor_joining(matrix, kind=kind, symmetrize=symmetrize, fill=fill, engine=engine)
    if labels is not None:
        tree = tree._replace(labels=_labels(labels, tree.n))
    text = tree.newick()
    if not write_output:
        return TreeRun(tree, text, None, None)
    if outdir is None:
        raise ValueError("run_tree needs outdir to write its files (or write_output=False)")
    out = Path(outdir) / "tree_output"
    out.mkdir(parents=True, exist_ok=True)
    newick_path, edges_path = out / f"{stem}_nj.nwk", out / f"{stem}_nj_edges.tab"
    newick_path.write_text(text + "\n")
    edges_frame(tree).to_csv(edges_path, index=False, sep="\t")
    return TreeRun(tree, text, newick_path, edges_path)
