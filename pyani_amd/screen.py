"""The screen: which of the N^2 ordered pairs of a collection are worth an exact comparison (the "k-mer sketch
pre-filter").  One engine call (Engine.screen_matrix, pg_screen_matrix) gives two INTEGER arrays for all genomes at once —
sizes[a] = |S(a)|, the distinct sampled canonical k-mers of genome a (FracMinHash: mix32(k-mer) & (scale - 1) == 0), and
shared[a][b] = |S(a) & S(b)| — and everything floating-point is computed here, on the host, from those integers:

    containment[a][b] = shared[a][b] / sizes[a]                        (NaN where sizes[a] == 0; the query on the rows)
    jaccard[a][b]     = shared[a][b] / (sizes[a] + sizes[b] - shared[a][b])
    identity[a][b]    = containment[a][b] ** (1 / k)  where shared[a][b] >= min_shared, else 0.0

(a k-mer survives iff none of its k bases changed).  The floor min_shared (default 2) matters: ONE chance k-mer between two unrelated
genomes of a few thousand sampled k-mers would read as an identity above 0.5.

Screened runs (run_anim / run_anib with screen=...) do not bring the matrix back at all: the selection rule of candidate_pairs reduces
to ONE INTEGER COMPARISON per cell (identity_thresholds), which the engine applies on the device next to the matrix
(Engine.screen_candidates) so that only the kept pairs are read back (ScreenedPairs).

Which genomes BELONG TOGETHER is the last step: the connected components of the kept pairs (components_of_pairs is
the statement, Engine.screen_components / screen_index_components the kernels, ScreenComponents the table: one representative per
component is the SINGLE-LINKAGE dereplicated set), had through the index without a single pair leaving the device
(Engine.screen_components_of).  One genome per SPECIES is the greedy rule of dRep, galah, skani and CD-HIT:
representatives_of_pairs is the statement, Engine.screen_representatives / screen_index_representatives the kernels, ScreenClusters the
table, Engine.screen_dereplicate the whole step.  dRep's SECONDARY clustering — average or complete linkage inside every component, cut at
1 - ANI — is linkage_of_pairs (the statement), Engine.screen_linkage (the kernels) and ScreenLinkage.

New genomes against a resident collection: Engine.screen_search lists what each is RELATED TO (SearchHits), and
Engine.screen_gather what each is MADE OF — the greedy minimum set of collection genomes that explains its k-mers (GatherOptions,
GatherResult).

An ESTIMATE for triage with its own frames: it is never written into an exact ANIm / ANIb matrix.  What this is modelled on: the
sketch-then-align front ends of skani, sourmash and dRep; pyani itself has no such step.
"""
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

DEFAULT_KMER, DEFAULT_SCALE, DEFAULT_MIN_SHARED = 16, 256, 2
MAX_GENOMES = 8192                 # screen_genomes: a dense ScreenResult
DENSE_MAX_GENOMES = 8192           # screen_candidates(path="auto"): the dense path up to here, the index path beyond (read at call time)
INDEX_MAX_GENOMES = 1 << 20        # the index path (Engine.screen_index)
MAX_BAND_ROWS, MAX_BAND_CELLS = 8192, 1 << 29
PATHS = ("auto", "dense", "index")


def default_band_rows(n: int) -> int:
    """The default band of the index path for n >= 1 genomes: the largest rows <= min(8192, n) with rows * n <= 2^29 cells."""
    if n < 1:
        raise ValueError("a band needs a genome")
    return min(MAX_BAND_ROWS, n, MAX_BAND_CELLS // n)


def default_search_rows(n: int) -> int:
    """The default chunk of queries of a search against n >= 1 db genomes: the largest rows <= 8192 with rows * n <= 2^29 cells (not capped
    by n: the rows are other genomes than the columns)."""
    if n < 1:
        raise ValueError("a search needs a db genome")
    return max(1, min(MAX_BAND_ROWS, MAX_BAND_CELLS // n))


def band_ranges(n: int, rows: int = 0) -> List[Tuple[int, int]]:
    """[(r0, r1)] of the bands of n genomes at the band setting `rows` (0 = the default): band b covers [b rows, min(n, (b + 1) rows))."""
    if n == 0:
        return []
    rows = int(rows) or default_band_rows(n)
    if not 1 <= rows <= MAX_BAND_ROWS:
        raise ValueError(f"a band is of 1 ... {MAX_BAND_ROWS} rows, not {rows}")
    return [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)]


def merge_dealt(parts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, shared) of the selections of dealt bands — part d holds the bands d, d + D, ..., each row-major — put back into global
    row-major order: concatenated, then a STABLE sort on the row.  A row lies in one band and so in one part, in column order."""
    a = np.concatenate([np.asarray(p[0], dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    b = np.concatenate([np.asarray(p[1], dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    s = np.concatenate([np.asarray(p[2], dtype=np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32)
    order = np.argsort(a, kind="stable")
    return a[order], b[order], s[order]


def resolve_path(path: str, n: int) -> str:
    """"dense" or "index" for a screen_candidates call over n genomes: "auto" is dense up to DENSE_MAX_GENOMES."""
    if path not in PATHS:
        raise ValueError(f"path must be one of {PATHS}, not {path!r}")
    if path == "auto":
        return "dense" if n <= DENSE_MAX_GENOMES else "index"
    return path


def check_params(kmer, scale) -> Tuple[int, int]:
    """(kmer, scale) as ints; ValueError outside 8 <= kmer <= 16 or for a scale that is no power of two in 1 ... 65536 (no library call)."""
    if isinstance(kmer, bool) or int(kmer) != kmer or not 8 <= int(kmer) <= 16:
        raise ValueError(f"the k-mer size must be an integer 8 ... 16, not {kmer!r}")
    if isinstance(scale, bool) or int(scale) != scale or not 1 <= int(scale) <= 65536 or int(scale) & (int(scale) - 1):
        raise ValueError(f"scale must be a power of two, 1 ... 65536, not {scale!r}")
    return int(kmer), int(scale)


class ScreenOptions(NamedTuple):
    """What a screened run asks of the screen: keep a pair iff its identity estimate, from either side, is >= min_identity.  There is
    no default threshold (on C4 0.80 kept every covered pair, 0.85 already lost relatives)."""
    min_identity: float
    kmer: int = DEFAULT_KMER
    scale: int = DEFAULT_SCALE
    min_shared: int = DEFAULT_MIN_SHARED


def check_options(options) -> ScreenOptions:
    """A ScreenOptions, or a bare number meaning min_identity, validated (no library call): kmer and scale as check_params, min_shared an
    integer >= 1 (the NaN rows of min_shared = 0 are not carried into the integer rule), min_identity a real number that is not NaN."""
    if not isinstance(options, ScreenOptions):
        if isinstance(options, bool) or not isinstance(options, (int, float, np.integer, np.floating)):
            raise ValueError(f"screen options are a ScreenOptions or a number (the identity threshold), not {options!r}")
        options = ScreenOptions(options)
    t = options.min_identity
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or math.isnan(float(t)):
        raise ValueError(f"min_identity must be a number, not {t!r}")
    kmer, scale = check_params(options.kmer, options.scale)
    ms = options.min_shared
    if isinstance(ms, bool) or not isinstance(ms, (int, np.integer)) or int(ms) < 1:
        raise ValueError(f"min_shared must be an integer >= 1, not {ms!r}")
    return ScreenOptions(float(t), kmer, scale, int(ms))


def _identity_of_counts(s: np.ndarray, size: np.ndarray, kmer: int) -> np.ndarray:
    """The expression of ScreenResult._identity for integer counts s of rows of `size` sampled k-mers (size > 0): numpy's own division
    and power on float64 arrays, so that the bits are those candidate_pairs compares."""
    return np.power(s.astype(np.float64) / size.astype(np.float64), 1.0 / kmer)


def identity_thresholds(sizes, kmer: int, min_identity: float, min_shared: int = DEFAULT_MIN_SHARED) -> np.ndarray:
    """need uint32[n]: need[a] = the smallest integer s with min_shared <= s <= sizes[a] and (s / sizes[a]) ** (1 / kmer) >= min_identity,
    in the float64 arithmetic of ScreenResult.identity; sizes[a] + 1 where there is none (an empty genome included); all 0 where
    min_identity <= 0.  For a fixed row the identity is monotone in the shared count, so identity[a][b] >= min_identity iff
    shared[a][b] >= need[a], and candidate_pairs' rule becomes: keep (a, b) iff a != b and shared[a][b] >= min(need[a], need[b])
    (what the monotonicity rests on).  Found by bisection over s with the very numpy expression of the identity."""
    kmer, _ = check_params(kmer, 1)
    if isinstance(min_shared, bool) or int(min_shared) != min_shared or int(min_shared) < 1:
        raise ValueError(f"min_shared must be an integer >= 1, not {min_shared!r}")
    t = float(min_identity)
    if math.isnan(t):
        raise ValueError("min_identity must be a number")
    size = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1)
    if (size < 0).any() or (size >= 2 ** 32 - 1).any():
        raise ValueError("sizes must fit uint32")
    if t <= 0.0:
        return np.zeros(len(size), dtype=np.uint32)
    need = size + 1
    lo = np.full(len(size), int(min_shared), dtype=np.int64)
    live = np.flatnonzero(lo <= size)
    if len(live):      # rows whose largest count passes: the answer lies in [lo, hi], and hi always passes
        live = live[_identity_of_counts(size[live], size[live], kmer) >= t]
    lo, hi, sz = lo[live], size[live], size[live]
    while True:
        open_ = lo < hi
        if not open_.any():
            break
        mid = (lo + hi) // 2
        ok = _identity_of_counts(mid, sz, kmer) >= t
        hi = np.where(open_ & ok, mid, hi)
        lo = np.where(open_ & ~ok, mid + 1, lo)
    need[live] = hi
    return need.astype(np.uint32)


class ScreenedPairs(NamedTuple):
    """The pairs a screen kept (Engine.screen_candidates), row-major — the order of ScreenResult.candidate_pairs — and nothing of the
    others: positions a, b in `labels`, shared = shared[a][b]."""
    labels: List[str]
    options: ScreenOptions
    sizes: np.ndarray       # uint32[n]
    a: np.ndarray           # int32[m]
    b: np.ndarray           # int32[m]
    shared: np.ndarray      # uint32[m]

    def pairs(self) -> List[Tuple[int, int]]:
        return list(zip(self.a.tolist(), self.b.tolist()))

    def containment(self) -> np.ndarray:
        """shared[a][b] / sizes[a] of the kept pairs (NaN where sizes[a] == 0)."""
        size = self.sizes.astype(np.float64)[self.a]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(size > 0, self.shared.astype(np.float64) / size, np.nan)

    def identity(self) -> np.ndarray:
        """ScreenResult.identity's value of the kept pairs: containment ** (1 / k) where shared >= min_shared, else 0.0."""
        ok = self.shared >= self.options.min_shared
        return np.where(ok, np.power(np.where(ok, self.containment(), 1.0), 1.0 / self.options.kmer), 0.0)

    def frame(self) -> pd.DataFrame:
        """One row per kept pair: query, subject (labels), shared, containment, identity."""
        lab = np.array(list(self.labels), dtype=object)
        return pd.DataFrame({"query": lab[self.a] if len(self.a) else [], "subject": lab[self.b] if len(self.b) else [], "shared": self.shared,
                             "containment": self.containment(), "identity": self.identity()})

    def components(self, engine=None) -> "ScreenComponents":
        """The connected components of the kept pairs: on `engine` (Engine.screen_components), or by the numpy statement
        components_of_pairs when none is given.  Both give the same ScreenComponents."""
        n = len(self.labels)
        if n == 0:
            return components_from_nodes(self.labels, np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
        nodes = components_of_pairs(self.a, self.b, self.shared, n) if engine is None else engine.screen_components(self.a, self.b, self.shared, n=n)
        return components_from_nodes(self.labels, *nodes)

    def representatives(self, scores=None, engine=None) -> "ScreenClusters":
        """The greedy clusters of the kept pairs, weight = shared: on `engine` (Engine.screen_representatives), or by
        the numpy statement representatives_of_pairs when none is given.  scores: one per genome, in the order of `labels`, as
        score_keys takes them; None = the sketch sizes.  Both give the same ScreenClusters."""
        n = len(self.labels)
        score = score_keys(scores, self.sizes)
        if len(score) != n:
            raise ValueError(f"{n} genomes need {n} scores, not {len(score)}")
        if n == 0:
            return clusters_from_nodes(self.labels, np.zeros(0, np.int32), np.zeros(0, np.uint32), score)
        if engine is None:
            rep, via = representatives_of_pairs(self.a, self.b, self.shared, n, score)
        else:
            rep, via = engine.screen_representatives(self.a, self.b, self.shared, n=n, score=score)
        return clusters_from_nodes(self.labels, rep, via, score)

    def evaluate(self, label, scores=None, engine=None) -> "ScreenEvaluation":
        """How good the partition `label` (check_partition: rep of .representatives(), root of .components(), ...) of the kept pairs
        is, weight = shared: on `engine` (Engine.screen_evaluate), or by the numpy statement evaluate_of_pairs when
        none is given.  scores as .representatives takes them.  Both give the same ScreenEvaluation."""
        n = len(self.labels)
        score = score_keys(scores, self.sizes)
        if len(score) != n:
            raise ValueError(f"{n} genomes need {n} scores, not {len(score)}")
        label = check_partition(label, n)
        if n == 0:
            return evaluation_from_nodes(self.labels, label, score, [np.zeros(0)] * 7, [np.zeros(0)] * 7)
        if engine is None:
            nodes, clusters = evaluate_of_pairs(self.a, self.b, self.shared, n, label, score)
        else:
            nodes, clusters = engine.screen_evaluate(self.a, self.b, self.shared, n=n, label=label, score=score)
        return evaluation_from_nodes(self.labels, label, score, nodes, clusters)

    def sweep(self, identities, snapshots=(), engine=None) -> "ScreenSweep":
        """The components of the kept pairs at every identity of a ladder: levels by sweep_thresholds + sweep_levels,
        then ONE pass on `engine` (Engine.screen_sweep), or the numpy statement sweep_of_pairs when none is given.  Both give the same
        ScreenSweep.  The ladder must start at or above options.min_identity (ValueError): these are the pairs kept THERE, and a lower
        step would miss pairs this list never held.  snapshots: at most 32 steps whose node arrays are kept (ScreenSweep.components_at)."""
        t = check_ladder(identities)
        if t[0] < self.options.min_identity:
            raise ValueError(f"the ladder starts at {t[0]!r}, below the {self.options.min_identity!r} these pairs were kept at")
        snaps = check_snapshots(snapshots, len(t))
        n = len(self.labels)
        need = sweep_thresholds(self.sizes, self.options.kmer, t, self.options.min_shared)
        level = sweep_levels(self.a, self.b, self.shared, need)
        if engine is None:
            arrays = sweep_of_pairs(self.a, self.b, level, n, len(t), self.shared, snaps)
        else:
            arrays = engine.screen_sweep(self.a, self.b, self.shared, level, n=n, steps=len(t), snapshots=snaps)
        return sweep_from_arrays(self.labels, t, arrays, snaps)


# ---- the connected components of the kept pairs ---------------------------------------------------------------------------
def _check_entries(a, b, shared, n):
    n = int(n)
    if not 1 <= n <= INDEX_MAX_GENOMES:
        raise ValueError(f"components are of 1 ... {INDEX_MAX_GENOMES} nodes, not {n}")
    a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.int64).reshape(-1)
    s = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32).reshape(-1)
    if len(a) != len(b) or (s is not None and len(s) != len(a)):
        raise ValueError("a, b and shared must have the same length")
    if len(a) and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n):
        raise ValueError(f"an entry names a node outside [0, {n})")
    return a, b, s, n


def components_of_pairs(a, b, shared, n) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """THE STATEMENT of the components (the host's; Engine.screen_components is held to it): for the list of entries (a[e], b[e], shared[e])
    over n nodes — unsorted, a pair in one direction or both, an entry once or several times; shared=None counts 1 everywhere — the three
    node arrays

        root[v]    int32   the smallest node of v's connected component (direction ignored)
        entries[v] uint64  the entries with a[e] == v and a[e] != b[e]
        weight[v]  uint64  the sum of shared[e] over those entries

    An entry with a[e] == b[e] is ignored altogether.  Integers, independent of the list's order.  Rounds of hooking every entry's larger
    root under its smaller one (np.minimum.at) and pointer jumping to the fixed point, until no entry joins two trees: a pointer only
    ever goes to a smaller node, so a tree's root is its smallest node, and the trees are the components."""
    a, b, s, n = _check_entries(a, b, shared, n)
    live = a != b
    a, b = a[live], b[live]
    entries = np.bincount(a, minlength=n).astype(np.uint64)
    if s is None:
        weight = entries.copy()
    else:      # float64 sums of 16-bit halves: exact below 2^37 entries
        s = s[live]
        lo = np.bincount(a, weights=(s & np.uint32(0xFFFF)).astype(np.float64), minlength=n).astype(np.uint64)
        hi = np.bincount(a, weights=(s >> np.uint32(16)).astype(np.float64), minlength=n).astype(np.uint64)
        weight = lo + (hi << np.uint64(16))
    root = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = root[a], root[b]
        join = ra != rb
        if not join.any():
            break
        a, b, ra, rb = a[join], b[join], ra[join], rb[join]      # (an entry inside one tree stays inside it: it is not looked at again)
        np.minimum.at(root, np.maximum(ra, rb), np.minimum(ra, rb))      # (what is hooked is a root: root[r] == r before)
        while True:
            up = root[root]
            if (up == root).all():
                break
            root = up
    return root.astype(np.int32), entries, weight


class ScreenComponents(NamedTuple):
    """The connected components of a list of kept pairs over the genomes `labels` (None: the nodes go by their index).  root, entries and
    weight are the node arrays of components_of_pairs; everything else is derived from them by components_from_nodes: components numbered
    by ascending root, members ascending inside a component."""
    labels: Optional[List[str]]
    root: np.ndarray             # int32[n]
    entries: np.ndarray          # uint64[n]
    weight: np.ndarray           # uint64[n]
    component: np.ndarray        # int32[n]: the component of every node
    start: np.ndarray            # int64[C + 1]: component c owns member[start[c]:start[c + 1]]
    member: np.ndarray           # int32[n]
    size: np.ndarray             # int64[C]
    edges: np.ndarray            # uint64[C]: the sum of `entries` over the members (ordered pairs, for a list that holds both directions)
    complete: np.ndarray         # bool[C]: edges == size (size - 1) — every ordered pair of members was kept; meaningful for a duplicate-free list
    representative: np.ndarray   # int32[C]: the member of the greatest weight, ties to the smallest index; a singleton represents itself

    def _names(self, nodes) -> list:
        nodes = np.asarray(nodes)
        return nodes.tolist() if self.labels is None else [self.labels[i] for i in nodes.tolist()]

    def members(self, c: int) -> np.ndarray:
        """The nodes of component c, ascending."""
        if not 0 <= int(c) < len(self.size):
            raise IndexError(f"component {c} does not exist ({len(self.size)} components)")
        return self.member[int(self.start[c]):int(self.start[c + 1])]

    def frame(self) -> pd.DataFrame:
        """One row per component: component, size, representative (label), edges, complete."""
        return pd.DataFrame({"component": np.arange(len(self.size), dtype=np.int64), "size": self.size, "representative": self._names(self.representative),
                             "edges": self.edges, "complete": self.complete})

    def membership_frame(self) -> pd.DataFrame:
        """One row per genome, in the order of `labels`: genome, component, representative (of its component)."""
        return pd.DataFrame({"genome": self._names(np.arange(len(self.root))), "component": self.component.astype(np.int64),
                             "representative": self._names(self.representative[self.component])})

    def representatives(self) -> list:
        """The single-linkage dereplicated set: one label per component, in component order (the greedy one: ScreenClusters)."""
        return self._names(self.representative)


def components_from_nodes(labels, root, entries, weight) -> ScreenComponents:
    """The ScreenComponents of the three node arrays (numpy on the host: n <= 2^20)."""
    root = np.ascontiguousarray(root, dtype=np.int32)
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    weight = np.ascontiguousarray(weight, dtype=np.uint64)
    n = len(root)
    if labels is not None:
        labels = [str(x) for x in labels]
        if len(labels) != n:
            raise ValueError("labels and nodes must have the same length")
    if len(entries) != n or len(weight) != n:
        raise ValueError("root, entries and weight must have the same length")
    if n == 0:
        z = np.zeros(0, np.int32)
        return ScreenComponents(labels, root, entries, weight, z, np.zeros(1, np.int64), z, np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros(0, bool), z)
    node = np.arange(n, dtype=np.int64)
    if (root < 0).any() or (root > node).any() or (root[root] != root).any():
        raise ValueError("root is no flattened forest (root[v] <= v and root[root[v]] == root[v])")
    _, component = np.unique(root, return_inverse=True)      # (ascending roots: the numbering)
    component = component.reshape(-1)
    size = np.bincount(component).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    member = np.argsort(component, kind="stable")
    edges = np.add.reduceat(entries[member], start[:-1])      # (every component has a member: no empty slice)
    sz = size.astype(np.uint64)
    complete = edges == sz * (sz - np.uint64(1))
    best = np.lexsort((node, ~weight, component))      # by component, then weight descending (~ reverses uint64), then index ascending
    return ScreenComponents(labels, root, entries, weight, component.astype(np.int32), start, member.astype(np.int32), size, edges, complete,
                            best[start[:-1]].astype(np.int32))


def merge_components(parts, n, engine=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(root, entries, weight) of the whole list from the node arrays of its PARTS — parts[d] = (root_d, entries_d, weight_d) of some of
    the entries, e.g. of the bands dealt to device d.  entries and weight add.  Each part is a forest of its own entries; the forests are
    joined by ONE list call over the entries (v, root_d[v]) with root_d[v] != v of every part (engine.screen_components, or the statement
    when no engine is given): v is connected to root_d[v] in part d, and every connection of part d runs through such entries."""
    n = int(n)
    entries, weight = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    va, vb = [], []
    for root, e, w in parts:
        root = np.ascontiguousarray(root, dtype=np.int32)
        if len(root) != n or len(e) != n or len(w) != n:
            raise ValueError(f"a part is not of {n} nodes")
        entries += np.asarray(e, dtype=np.uint64)
        weight += np.asarray(w, dtype=np.uint64)
        v = np.flatnonzero(root != np.arange(n, dtype=np.int32)).astype(np.int32)
        va.append(v)
        vb.append(root[v])
    a = np.concatenate(va) if va else np.zeros(0, np.int32)
    b = np.concatenate(vb) if vb else np.zeros(0, np.int32)
    root = (components_of_pairs(a, b, None, n) if engine is None else engine.screen_components(a, b, None, n=n))[0]
    return root, entries, weight


def index_components_on(engines, run_all, ids, options, labels=None) -> ScreenComponents:
    """The components through the index on the D engines given, without a pair leaving a device: every engine builds the index, engine d
    hooks and accumulates the kept cells of the bands d, d + D, ... (Engine.screen_index_components), and the parts are joined by
    merge_components on the first engine; the indexes and the parts' resident results are released, on errors too.  run_all as for
    index_candidates_on.  Equal to index_candidates_on(...).components()."""
    options = check_options(options)
    ids = list(ids)
    labels = _labels_for(ids, labels, INDEX_MAX_GENOMES)
    if not ids:
        return components_from_nodes(labels, np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    d = len(engines)

    def part(engine, k):
        sizes = engine.screen_index(ids, options.kmer, options.scale)
        need = identity_thresholds(sizes, options.kmer, options.min_identity, options.min_shared)
        return engine.screen_index_components(need, band_first=k, band_step=d)[:3]
    try:
        parts = run_all(part)
        nodes = parts[0] if d == 1 else merge_components(parts, len(ids), engine=engines[0])
    finally:
        for e in engines:
            e.screen_index_release()
            e.screen_components_release()
    return components_from_nodes(labels, *nodes)


# ---- the sweep: the components over a ladder of thresholds ------------------------------------------------------------------
SWEEP_MAX_STEPS = 4096
SWEEP_MAX_SNAPSHOTS = 32
SWEEP_MAX_TABLE = 1 << 28          # words of the need table the index form takes (Engine.screen_index_sweep)


def check_ladder(identities) -> np.ndarray:
    """A ladder: 1 ... SWEEP_MAX_STEPS identities as float64, none NaN, STRICTLY ascending (ValueError otherwise)."""
    t = np.ascontiguousarray(identities, dtype=np.float64).reshape(-1)
    if not 1 <= len(t) <= SWEEP_MAX_STEPS:
        raise ValueError(f"a ladder has 1 ... {SWEEP_MAX_STEPS} steps, not {len(t)}")
    if np.isnan(t).any() or (np.diff(t) <= 0).any():
        raise ValueError("a ladder's identities must be numbers in strictly ascending order")
    return t


def check_snapshots(snapshots, steps: int) -> List[int]:
    snaps = [int(s) for s in snapshots]
    if len(snaps) > SWEEP_MAX_SNAPSHOTS:
        raise ValueError(f"a sweep keeps at most {SWEEP_MAX_SNAPSHOTS} snapshots, not {len(snaps)}")
    if any(not 0 <= s < steps for s in snaps):
        raise ValueError(f"a snapshot step lies outside [0, {steps})")
    return snaps


def sweep_thresholds(sizes, kmer: int, identities, min_shared: int = DEFAULT_MIN_SHARED) -> np.ndarray:
    """need uint32[S][n]: row s = identity_thresholds(sizes, kmer, T_s, min_shared) for the ladder T_0 < ... < T_{S-1} (check_ladder).
    Every column is non-decreasing in s — a higher identity never asks for fewer shared k-mers; this is checked, ValueError otherwise —
    so the graphs of the steps are nested."""
    t = check_ladder(identities)
    need = np.stack([identity_thresholds(sizes, kmer, float(x), min_shared) for x in t])
    check_need_table(need)
    return need


def check_need_table(need) -> np.ndarray:
    need = np.asarray(need)
    if need.ndim != 2 or not 1 <= need.shape[0] <= SWEEP_MAX_STEPS:
        raise ValueError(f"a need table is uint32[steps][n] with 1 ... {SWEEP_MAX_STEPS} steps")
    if need.shape[0] > 1 and (need[1:] < need[:-1]).any():
        raise ValueError("a need table's columns must not fall from one step to the next")
    return need


def sweep_levels(a, b, shared, need) -> np.ndarray:
    """level uint16[m] of the entries (a, b, shared) under the table `need` of sweep_thresholds: the number of leading steps that keep
    the entry — the smallest s with shared < min(need[s][a], need[s][b]), or S when there is none.  The entry is present at step s iff
    level > s, which is the very rule screen_candidates applies at T_s."""
    need = check_need_table(need)
    a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.int64).reshape(-1)
    s = np.ascontiguousarray(shared, dtype=np.uint32).reshape(-1)
    if len(a) != len(b) or len(s) != len(a):
        raise ValueError("a, b and shared must have the same length")
    level = np.zeros(len(a), dtype=np.uint16)
    alive = np.arange(len(a))      # the entries every step so far has kept
    for row in need:
        if not len(alive):
            break
        alive = alive[s[alive] >= np.minimum(row[a[alive]], row[b[alive]])]
        level[alive] += np.uint16(1)
    return level


def levels_of_values(values, thresholds) -> np.ndarray:
    """level uint16[m] of any float weight under a ladder of thresholds (check_ladder): the number of thresholds <= value, NaN giving 0 —
    present at step s iff value >= thresholds[s].  With it a list of exact identities can be swept as well."""
    t = check_ladder(thresholds)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    level = np.searchsorted(t, v, side="right")
    level[np.isnan(v)] = 0
    return level.astype(np.uint16)


def sweep_of_pairs(a, b, level, n, steps, shared=None, snapshots=()):
    """THE STATEMENT of the sweep (the host's; Engine.screen_sweep is held to it): the list of entries (a[e], b[e], shared[e]) is that
    of components_of_pairs, and entry e is present at step s iff level[e] > s (0 <= level[e] <= steps).  For every step s of
    0 ... steps - 1, over the entries with a != b present at s:

        entries[s]    uint64  their number
        components[s] uint32  the connected components over all n nodes, singletons included
        singletons[s] uint32  the components of one node
        largest[s]    uint32  the size of the largest component
        pair_slots[s] uint64  the sum over the components of size * (size - 1)

    and for every step of `snapshots` the (root, entries, weight) of components_of_pairs on the entries present there.  Returns
    (entries, components, singletons, largest, pair_slots, [node arrays per snapshot]).  One components_of_pairs call per step: slow,
    obvious, and independent of the device's single pass."""
    a, b, s, n = _check_entries(a, b, shared, n)
    steps = int(steps)
    if not 1 <= steps <= SWEEP_MAX_STEPS:
        raise ValueError(f"a sweep has 1 ... {SWEEP_MAX_STEPS} steps, not {steps}")
    level = np.ascontiguousarray(level, dtype=np.int64).reshape(-1)
    if len(level) != len(a):
        raise ValueError("a, b and level must have the same length")
    if len(level) and (level.min() < 0 or level.max() > steps):
        raise ValueError(f"a level lies outside [0, {steps}]")
    snaps = check_snapshots(snapshots, steps)
    entries, pair_slots = np.zeros(steps, dtype=np.uint64), np.zeros(steps, dtype=np.uint64)
    components, singletons, largest = (np.zeros(steps, dtype=np.uint32) for _ in range(3))
    nodes_at = {}
    for step in range(steps):
        here = level > step
        nodes = components_of_pairs(a[here], b[here], None if s is None else s[here], n)
        size = np.bincount(nodes[0], minlength=n).astype(np.uint64)
        size = size[size > 0]
        entries[step] = int((a[here] != b[here]).sum())
        components[step], singletons[step], largest[step] = len(size), int((size == 1).sum()), int(size.max())
        pair_slots[step] = int((size * (size - np.uint64(1))).sum())
        if step in snaps:
            nodes_at[step] = nodes
    return entries, components, singletons, largest, pair_slots, [nodes_at[k] for k in snaps]


class ScreenSweep(NamedTuple):
    """The components of a list of entries over a ladder of identities: one value per step of every array of
    sweep_of_pairs, complete = (pair_slots == entries) — for a duplicate-free list that holds both directions, such as a selection,
    "every component is a clique", the sense of ScreenComponents.complete — and the node arrays of the snapshot steps."""
    labels: Optional[List[str]]
    identities: np.ndarray       # float64[S], ascending
    entries: np.ndarray          # uint64[S]
    components: np.ndarray       # uint32[S]
    singletons: np.ndarray       # uint32[S]
    largest: np.ndarray          # uint32[S]
    pair_slots: np.ndarray       # uint64[S]
    complete: np.ndarray         # bool[S]
    snapshot_steps: List[int]
    snapshots: list              # [(root, entries, weight)] in the order of snapshot_steps

    def frame(self) -> pd.DataFrame:
        """One row per step: step, identity, entries, components, singletons, largest, pair_slots, complete."""
        return pd.DataFrame({"step": np.arange(len(self.identities), dtype=np.int64), "identity": self.identities, "entries": self.entries,
                             "components": self.components, "singletons": self.singletons, "largest": self.largest, "pair_slots": self.pair_slots,
                             "complete": self.complete})

    def special(self) -> pd.DataFrame:
        """The steps at which every component is a clique (classify.special_intervals' sense): the rows of frame() with `complete`."""
        return self.frame()[self.complete].reset_index(drop=True)

    def components_at(self, step: int) -> ScreenComponents:
        """The ScreenComponents of a SNAPSHOT step (IndexError for any other step: its node arrays were not kept)."""
        if int(step) not in self.snapshot_steps:
            raise IndexError(f"step {step} is no snapshot of this sweep (snapshots: {self.snapshot_steps})")
        return components_from_nodes(self.labels, *self.snapshots[self.snapshot_steps.index(int(step))])


def sweep_from_arrays(labels, identities, arrays, snapshot_steps) -> ScreenSweep:
    """The ScreenSweep of what sweep_of_pairs or Engine.screen_sweep returned."""
    entries, components, singletons, largest, pair_slots, snapshots = arrays
    t = check_ladder(identities)
    if any(len(x) != len(t) for x in (entries, components, singletons, largest, pair_slots)):
        raise ValueError("the ladder and the per-step arrays must have the same length")
    entries, pair_slots = np.ascontiguousarray(entries, dtype=np.uint64), np.ascontiguousarray(pair_slots, dtype=np.uint64)
    return ScreenSweep(None if labels is None else [str(x) for x in labels], t, entries, np.ascontiguousarray(components, dtype=np.uint32),
                       np.ascontiguousarray(singletons, dtype=np.uint32), np.ascontiguousarray(largest, dtype=np.uint32), pair_slots,
                       pair_slots == entries, [int(s) for s in snapshot_steps], list(snapshots))


# ---- the greedy representatives of the kept pairs ---------------------------------------------------------------------------
def score_keys(scores, sizes=None) -> np.ndarray:
    """uint64 keys of the genomes' scores, greater is better.  scores=None: the sketch sizes (ScreenedPairs.sizes), so that the larger
    assembly wins.  Otherwise the scores must be float64-convertible, finite and >= 0 (ValueError), and the key is the bit pattern of
    x + 0.0 (the addition turns -0.0 into 0.0), which is monotone for non-negative doubles."""
    if scores is None:
        if sizes is None:
            raise ValueError("no scores and no sizes to take their place")
        return np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1).copy()
    try:
        x = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as err:
        raise ValueError(f"scores must be numbers: {err}") from None
    if not np.isfinite(x).all() or (x < 0).any():
        raise ValueError("scores must be finite and >= 0")
    return (x + 0.0).view(np.uint64).copy()


def rank_order(score) -> Tuple[np.ndarray, np.ndarray]:
    """(order, rank) of uint64 scores: order = the nodes by (score descending, index ascending), rank its inverse."""
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    order = np.lexsort((np.arange(len(score)), ~score))
    rank = np.empty(len(score), dtype=np.int64)
    rank[order] = np.arange(len(score))
    return order, rank


def representatives_of_pairs(a, b, weight, n, score) -> Tuple[np.ndarray, np.ndarray]:
    """THE STATEMENT of the representatives (the host's; Engine.screen_representatives is held to it): for the list of entries
    (a[e], b[e], weight[e]) over n nodes — unsorted, a pair in one direction or both, once or several times, an entry with a[e] == b[e]
    ignored, weight=None counting 1 everywhere — and the scores score uint64[n] (greater is better, ties to the smaller index; order,
    rank = rank_order(score)):

      1. Walk `order`.  A node none of whose neighbours is already a representative becomes one.  Direction is ignored.
      2. Every other node v is assigned to the representative neighbour r of the greatest pair weight — the maximum of weight[e] over
         all entries joining v and r, in either direction — ties to the representative of smaller rank.

    The assignment is made AFTER all representatives are known (galah's rule), not as CD-HIT does during the walk ("the first
    representative met"): a representative of lower priority than v may take v.  The two differ already on chains, so the two-phase
    form is deliberate.  Returns rep int32[n] (rep[v] == v for a representative) and via uint32[n] (the pair weight v was assigned by, 0
    for a representative).  Integers, independent of the list's order, direction and duplication.

    The walk is the lexicographically first maximal independent set under `rank`; it is computed here in rounds over the entries whose
    ends are both undecided: the end of larger rank of each is barred, every undecided node not barred becomes a representative (all
    its neighbours of higher priority have been covered), and the undecided neighbours of the new representatives are covered.  The
    undecided node of smallest rank is never barred, so every round decides a node."""
    a, b, w, n = _check_entries(a, b, weight, n)
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    if len(score) != n:
        raise ValueError(f"{n} nodes need {n} scores, not {len(score)}")
    order, rank = rank_order(score)
    live = a != b
    a, b = a[live], b[live]
    w = np.ones(len(a), dtype=np.uint64) if w is None else w[live].astype(np.uint64)
    is_rep, covered = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    ea, eb = a, b
    while True:
        undecided = ~(is_rep | covered)
        if not undecided.any():
            break
        both = undecided[ea] & undecided[eb]      # (an entry with a decided end is never looked at again: nothing becomes undecided)
        ea, eb = ea[both], eb[both]
        barred = np.zeros(n, dtype=bool)
        barred[np.where(rank[ea] > rank[eb], ea, eb)] = True
        new = undecided & ~barred
        is_rep |= new
        covered[eb[new[ea]]] = True
        covered[ea[new[eb]]] = True
    # the assignment: per covered node the greatest (weight, -rank of the representative) over the entries that join it to a representative
    fwd, bwd = is_rep[a] & covered[b], is_rep[b] & covered[a]
    v = np.concatenate([b[fwd], a[bwd]])
    r = np.concatenate([a[fwd], b[bwd]])
    key = (np.concatenate([w[fwd], w[bwd]]) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rank[r].astype(np.uint64))
    by = np.lexsort((key, v))
    v, key = v[by], key[by]
    last = np.flatnonzero(np.append(v[1:] != v[:-1], True)) if len(v) else np.zeros(0, np.int64)      # the greatest key of every covered node
    rep = np.arange(n, dtype=np.int64)
    via = np.zeros(n, dtype=np.uint32)
    rep[v[last]] = order[(np.uint64(0xFFFFFFFF) - (key[last] & np.uint64(0xFFFFFFFF))).astype(np.int64)]
    via[v[last]] = (key[last] >> np.uint64(32)).astype(np.uint32)
    return rep.astype(np.int32), via


class ScreenClusters(NamedTuple):
    """The greedy clusters of a list of kept pairs over the genomes `labels` (None: the nodes go by their index).  rep, via and score are
    the node arrays of representatives_of_pairs and its scores; everything else is derived from them by clusters_from_nodes: clusters
    numbered by ascending representative, members ascending inside a cluster."""
    labels: Optional[List[str]]
    rep: np.ndarray              # int32[n]
    via: np.ndarray              # uint32[n]
    score: np.ndarray            # uint64[n]
    representative: np.ndarray   # int32[R]: ascending node index
    cluster: np.ndarray          # int32[n]: the cluster of every node
    start: np.ndarray            # int64[R + 1]: cluster c owns member[start[c]:start[c + 1]]
    member: np.ndarray           # int32[n]
    size: np.ndarray             # int64[R]

    def _names(self, nodes) -> list:
        nodes = np.asarray(nodes)
        return nodes.tolist() if self.labels is None else [self.labels[i] for i in nodes.tolist()]

    def members(self, c: int) -> np.ndarray:
        """The nodes of cluster c, ascending."""
        if not 0 <= int(c) < len(self.size):
            raise IndexError(f"cluster {c} does not exist ({len(self.size)} clusters)")
        return self.member[int(self.start[c]):int(self.start[c + 1])]

    def frame(self) -> pd.DataFrame:
        """One row per representative: cluster, representative (label), size, score (the uint64 key)."""
        return pd.DataFrame({"cluster": np.arange(len(self.size), dtype=np.int64), "representative": self._names(self.representative), "size": self.size,
                             "score": self.score[self.representative]})

    def membership_frame(self) -> pd.DataFrame:
        """One row per genome, in the order of `labels`: genome, representative, via."""
        return pd.DataFrame({"genome": self._names(np.arange(len(self.rep))), "representative": self._names(self.rep), "via": self.via.astype(np.int64)})

    def representatives(self) -> list:
        """The dereplicated set: one label per cluster, in cluster order."""
        return self._names(self.representative)


def clusters_from_nodes(labels, rep, via, score) -> ScreenClusters:
    """The ScreenClusters of the node arrays (numpy on the host: n <= 2^20)."""
    rep = np.ascontiguousarray(rep, dtype=np.int32).reshape(-1)
    via = np.ascontiguousarray(via, dtype=np.uint32).reshape(-1)
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    n = len(rep)
    if labels is not None:
        labels = [str(x) for x in labels]
        if len(labels) != n:
            raise ValueError("labels and nodes must have the same length")
    if len(via) != n or len(score) != n:
        raise ValueError("rep, via and score must have the same length")
    if n and ((rep < 0).any() or (rep >= n).any() or (rep[rep] != rep).any()):
        raise ValueError("rep names no representatives (0 <= rep[v] < n and rep[rep[v]] == rep[v])")
    representative, cluster = np.unique(rep, return_inverse=True)      # (ascending representatives: the numbering)
    cluster = cluster.reshape(-1)
    size = np.bincount(cluster, minlength=len(representative)).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    member = np.argsort(cluster, kind="stable")
    return ScreenClusters(labels, rep, via, score, representative.astype(np.int32), cluster.astype(np.int32), start, member.astype(np.int32), size)


# ---- species clusters by linkage inside every component ---------------------------------------------------------------------
LINKAGE_METHODS = ("average", "complete")
LINKAGE_MAX_COMPONENT = 8192       # Engine.screen_linkage: nodes of one component (the linkage kernel's own limit); the statement has none


def check_linkage(method, cutoff, fill) -> Tuple[str, float, float]:
    """(method, cutoff, fill) of a linkage call: the method one of LINKAGE_METHODS, cutoff and fill finite and >= 0, cutoff STRICTLY below
    fill (ValueError otherwise): an absent pair sits at `fill` and must never be joined by the cut."""
    if method not in LINKAGE_METHODS:
        raise ValueError(f"method must be one of {LINKAGE_METHODS}, not {method!r}")
    try:
        cutoff, fill = float(cutoff), float(fill)
    except (TypeError, ValueError) as err:
        raise ValueError(f"cutoff and fill must be numbers: {err}") from None
    if not (math.isfinite(cutoff) and math.isfinite(fill)) or cutoff < 0 or fill < 0:
        raise ValueError("cutoff and fill must be finite and >= 0")
    if not cutoff < fill:
        raise ValueError(f"cutoff ({cutoff!r}) must be strictly below fill ({fill!r})")
    return method, cutoff, fill


def check_distances(dist, m: int) -> np.ndarray:
    """The float64 distances of m entries: the array must BE float64 (no silent conversion: the bits are the statement's), finite, >= 0."""
    dist = np.asarray(dist)
    if dist.dtype != np.float64:
        raise ValueError(f"dist must be float64, not {dist.dtype}")
    dist = np.ascontiguousarray(dist).reshape(-1)
    if len(dist) != m:
        raise ValueError("a, b and dist must have the same length")
    if not np.isfinite(dist).all() or (dist < 0).any():
        raise ValueError("distances must be finite and >= 0")
    return dist + 0.0      # (-0.0 becomes 0.0: the bit pattern of a distance is then monotone)


def _chain_linkage(D: np.ndarray, average: bool) -> np.ndarray:
    """scipy's nearest-neighbour chain on the symmetric matrix D (changed in place): the s - 1 records (lower slot, higher slot, height,
    size) in merge order.  Ascending scan, strict <, lowest index wins; average as (n_lo a + n_hi b) / (n_lo + n_hi), every operation
    rounded on its own — what cluster_linkage_kernel does, in numpy's float64."""
    s = len(D)
    size = np.ones(s, dtype=np.int64)
    out = np.zeros((s - 1, 4), dtype=np.float64)
    chain: List[int] = []
    for k in range(s - 1):
        if not chain:
            chain.append(int(np.flatnonzero(size)[0]))
        while True:
            x = chain[-1]
            row = np.where(size > 0, D[x], np.inf)
            row[x] = np.inf
            y = int(np.argmin(row))      # (the first index attaining the minimum)
            cur = row[y]
            if len(chain) > 1:
                prev = chain[-2]
                if not cur < D[x, prev]:      # the incumbent stays unless strictly beaten
                    y, cur = prev, D[x, prev]
                if y == prev:
                    break
            chain.append(y)
        y, x = chain.pop(), chain.pop()
        lo, hi = (x, y) if x < y else (y, x)
        nlo, nhi = int(size[lo]), int(size[hi])
        out[k] = (lo, hi, cur, nlo + nhi)
        if average:
            new = (np.float64(nlo) * D[lo] + np.float64(nhi) * D[hi]) / np.float64(nlo + nhi)
        else:
            new = np.maximum(D[lo], D[hi])
        keep = size > 0
        keep[lo] = keep[hi] = False
        D[hi, keep] = new[keep]
        D[keep, hi] = new[keep]
        size[lo], size[hi] = 0, nlo + nhi
    return out


def linkage_of_pairs(a, b, dist, n, score, method: str = "average", cutoff: float = 0.05, fill: float = 1.0):
    """THE STATEMENT of the linkage (the host's; Engine.screen_linkage is held to it): for the list of entries (a[e], b[e], dist[e]) over n
    nodes — unsorted, a pair in one direction or both, once or several times, an entry with a[e] == b[e] ignored — and the scores score
    uint64[n] (score_keys):

      1. root[v] = the smallest node of v's connected component, as components_of_pairs gives it.  The local index of a node is its
         position among its component's members in ascending node order.
      2. Per component of s >= 2 nodes the matrix D: D[i][j] = the MAXIMUM of dist[e] over all entries joining the two nodes, in either
         direction (the order-independent counterpart of exact_edges' minimum identity); `fill` where no entry joins them (dRep treats an
         uncompared pair as ANI 0); 0 on the diagonal.
      3. scipy's nearest-neighbour chain on D for "average" or "complete" (_chain_linkage): the s - 1 merge records in merge order, which
         graphics.merges_to_linkage turns into scipy's Z.
      4. Two nodes share a cluster iff merges of height <= cutoff join them — fcluster(Z, cutoff, "distance"): both methods are monotone,
         so a union over those records is the whole rule.  cluster[v] = the smallest member of v's cluster.
      5. rep[v] = the member of v's cluster of the greatest score, ties to the smaller index.

    Returns root, cluster, rep (int32[n]) and merges float64[n - components, 4]: the components' blocks in ascending root order, slots as
    local indices.  Integers, and doubles whose bits the steps fix; nothing depends on the list's order, direction or duplication.
    ValueError before any work: check_distances, check_linkage.

    A property, tested and not assumed: absent pairs sit exactly at `fill` and cutoff < fill, and then the partition equals fcluster of ONE
    linkage over the whole n x n matrix with the absent cells at `fill`; the components only save the n^2 work."""
    a, b, _, n = _check_entries(a, b, None, n)
    dist = check_distances(dist, len(a))
    method, cutoff, fill = check_linkage(method, cutoff, fill)
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    if len(score) != n:
        raise ValueError(f"{n} nodes need {n} scores, not {len(score)}")
    live = a != b
    a, b, dist = a[live], b[live], dist[live]
    root = components_of_pairs(a, b, None, n)[0].astype(np.int64)
    order = np.lexsort((np.arange(n), root))      # by (root, node)
    heads = np.flatnonzero(root[order] == order)
    start = np.append(heads, n)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    comp = np.searchsorted(heads, pos, side="right") - 1      # of every node
    local = pos - start[comp]
    # the entries by component, each cell once: the maximum over both directions and every duplicate
    ec = comp[a]
    by = np.argsort(ec, kind="stable")
    ec, ei, ej, ed = ec[by], local[a][by], local[b][by], dist[by]
    cuts = np.searchsorted(ec, np.arange(len(heads) + 1))
    cluster = np.arange(n, dtype=np.int64)
    blocks = []
    for c in range(len(heads)):
        s = int(start[c + 1] - start[c])
        if s < 2:
            continue
        sl = slice(cuts[c], cuts[c + 1])
        D = np.full((s, s), -1.0)
        np.maximum.at(D, (ei[sl], ej[sl]), ed[sl])
        D = np.maximum(D, D.T)
        D[D < 0] = fill
        np.fill_diagonal(D, 0.0)
        rec = _chain_linkage(D, method == "average")
        blocks.append(rec)
        nodes = order[start[c]:start[c + 1]]
        label = np.arange(s)      # the cut: a union over the records of height <= cutoff, the smaller label taking the other's members
        for lo, hi, h, _ in rec:
            if h <= cutoff:
                x, y = label[int(lo)], label[int(hi)]
                if x != y:
                    label[label == max(x, y)] = min(x, y)
        cluster[nodes] = nodes[label]      # (a label is the smallest local index of its cluster; the members ascend with it)
    merges = np.concatenate(blocks) if blocks else np.zeros((0, 4), dtype=np.float64)
    best = np.lexsort((np.arange(n), ~score, cluster))      # by cluster, then score descending, then index ascending
    first = np.flatnonzero(np.append(True, cluster[best][1:] != cluster[best][:-1]))
    rep_of = np.empty(n, dtype=np.int64)
    rep_of[cluster[best][first]] = best[first]
    return root.astype(np.int32), cluster.astype(np.int32), rep_of[cluster].astype(np.int32), merges


class ScreenLinkage(NamedTuple):
    """The species clusters by linkage of a list of pairs with distances over the genomes `labels` (None: the nodes go by their index):
    the node arrays and merge records of linkage_of_pairs, its scores and its three parameters."""
    labels: Optional[List[str]]
    root: np.ndarray             # int32[n]
    cluster: np.ndarray          # int32[n]
    rep: np.ndarray              # int32[n]
    score: np.ndarray            # uint64[n]
    merges: np.ndarray           # float64[n - components, 4]
    method: str
    cutoff: float
    fill: float

    def clusters(self) -> "ScreenClusters":
        """The clusters as the greedy rule's table (clusters_from_nodes): representative, members, sizes; `via` is 0 everywhere."""
        return clusters_from_nodes(self.labels, self.rep, np.zeros(len(self.rep), dtype=np.uint32), self.score)

    def _blocks(self):
        """(roots ascending, start of every component among the nodes in (root, node) order, first merge record of every component)"""
        roots, size = np.unique(self.root, return_counts=True)
        return roots, np.concatenate([[0], np.cumsum(size)]), np.concatenate([[0], np.cumsum(size - 1)])

    def linkage_of(self, root: int) -> Tuple[np.ndarray, np.ndarray]:
        """(Z, members) of the component whose smallest node is `root`: scipy's linkage matrix (graphics.merges_to_linkage; 0 rows for a
        component of one node) and the member nodes in ascending order — leaf i of Z is members[i]."""
        from .graphics import merges_to_linkage
        roots, _, first = self._blocks()
        c = int(np.searchsorted(roots, int(root)))
        if c >= len(roots) or roots[c] != int(root):
            raise IndexError(f"node {root} is no component's root")
        members = np.flatnonzero(self.root == int(root)).astype(np.int32)
        block = self.merges[int(first[c]):int(first[c + 1])]
        return (merges_to_linkage(block) if len(block) else np.zeros((0, 4), dtype=np.float64)), members

    def frame(self) -> pd.DataFrame:
        """One row per cluster: cluster, representative (label), size, score (the uint64 key), component (the root's label)."""
        t = self.clusters()
        out = t.frame()
        out["component"] = t._names(self.root[t.representative])
        return out

    def merges_frame(self) -> pd.DataFrame:
        """One row per merge: component (the root's label), left, right, height, size — left and right in scipy's numbering (a leaf is its
        local index, the cluster made by row r of a component of s nodes is s + r)."""
        roots, _, first = self._blocks()
        comp, left, right, height, size = [], [], [], [], []
        for c, r in enumerate(roots.tolist()):
            if first[c + 1] == first[c]:
                continue
            Z, _ = self.linkage_of(r)
            comp += [r] * len(Z)
            left += Z[:, 0].astype(np.int64).tolist()
            right += Z[:, 1].astype(np.int64).tolist()
            height += Z[:, 2].tolist()
            size += Z[:, 3].astype(np.int64).tolist()
        names = comp if self.labels is None else [self.labels[i] for i in comp]
        return pd.DataFrame({"component": names, "left": left, "right": right, "height": height, "size": size})


def linkage_from_nodes(labels, root, cluster, rep, score, merges, method, cutoff, fill) -> ScreenLinkage:
    """The ScreenLinkage of what linkage_of_pairs or Engine.screen_linkage returned."""
    root, cluster, rep = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in (root, cluster, rep))
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    merges = np.ascontiguousarray(merges, dtype=np.float64).reshape(-1, 4)
    n = len(root)
    if labels is not None:
        labels = [str(x) for x in labels]
        if len(labels) != n:
            raise ValueError("labels and nodes must have the same length")
    if len(cluster) != n or len(rep) != n or len(score) != n:
        raise ValueError("root, cluster, rep and score must have the same length")
    if len(merges) != n - len(np.unique(root)):
        raise ValueError("the merge records do not match the components")
    method, cutoff, fill = check_linkage(method, cutoff, fill)
    return ScreenLinkage(labels, root, cluster, rep, score, merges, method, cutoff, fill)


# ---- the evaluation of a partition of the kept pairs -----------------------------------------------------------------------
EVALUATE_MAX_ENTRIES = 0xFFFFFFFF      # with at most 2^32 - 1 entries of uint32 weights no 64-bit sum can overflow
EVALUATE_NONE = 0xFFFFFFFF             # in_min / min of a node / cluster without an inside pair
EVALUATE_NODE_ARRAYS = ("in_pairs", "in_weight", "in_min", "out_pairs", "out_weight", "out_node", "to_medoid")
EVALUATE_CLUSTER_ARRAYS = ("size", "pairs", "weight", "min", "medoid", "near_weight", "near_cluster")
_EVALUATE_NODE_TYPES = (np.uint32, np.uint64, np.uint32, np.uint32, np.uint32, np.int32, np.uint32)
_EVALUATE_CLUSTER_TYPES = (np.uint32, np.uint64, np.uint64, np.uint32, np.int32, np.uint32, np.int32)


def check_partition(label, n: int) -> np.ndarray:
    """int64[n] of a partition given by naming nodes: 0 <= label[v] < n and label[label[v]] == label[v] (ValueError names the first node
    that breaks it).  rep of the representatives, cluster and rep of the linkage and root of the components all satisfy it."""
    try:
        label = np.ascontiguousarray(label, dtype=np.int64).reshape(-1)
    except (TypeError, ValueError) as err:
        raise ValueError(f"labels must be node indices: {err}") from None
    if len(label) != int(n):
        raise ValueError(f"{int(n)} nodes need {int(n)} labels, not {len(label)}")
    bad = (label < 0) | (label >= n)
    if bad.any():
        v = int(np.flatnonzero(bad)[0])
        raise ValueError(f"node {v} has the label {int(label[v])} outside [0, {int(n)})")
    bad = label[label] != label
    if bad.any():
        v = int(np.flatnonzero(bad)[0])
        raise ValueError(f"node {v} has the label {int(label[v])}, which does not name itself (label[label[v]] == label[v])")
    return label


def _sum_by(group, w, n) -> np.ndarray:
    """uint64[n]: the sum of the uint64 values w < 2^32 per group (float64 sums of 16-bit halves: exact below 2^37 entries)."""
    lo = np.bincount(group, weights=(w & np.uint64(0xFFFF)).astype(np.float64), minlength=n).astype(np.uint64)
    hi = np.bincount(group, weights=(w >> np.uint64(16)).astype(np.float64), minlength=n).astype(np.uint64)
    return lo + (hi << np.uint64(16))


def _pick_by(group, key, largest: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(groups, keys): per group that occurs, its largest or its smallest key (one lexsort; the run's last or first entry)."""
    if not len(group):
        return group, key
    by = np.lexsort((key, group))
    g, k = group[by], key[by]
    edge = g[1:] != g[:-1]
    at = np.flatnonzero(np.append(edge, True)) if largest else np.flatnonzero(np.append(True, edge))
    return g[at], k[at]


def evaluate_of_pairs(a, b, weight, n, label, score):
    """THE STATEMENT of the evaluation (the host's; Engine.screen_evaluate is held to it): for the list of entries (a[e], b[e], weight[e])
    over n nodes — unsorted, a pair in one direction or both, once or several times, an entry with a[e] == b[e] ignored, weight=None
    weighing every entry 1 —, a partition label (check_partition) and the scores score uint64[n] (rank = rank_order(score)[1]):

    A PAIR is a distinct unordered {u, v}, u != v, joined by at least one entry; its weight is the MAXIMUM of weight[e] over those
    entries, in either direction.  It is INSIDE iff label[u] == label[v], otherwise OUTSIDE.  Per node v (EVALUATE_NODE_ARRAYS):

        in_pairs[v]   uint32  the inside pairs at v
        in_weight[v]  uint64  the sum of their weights
        in_min[v]     uint32  the smallest of them, 0xFFFFFFFF when there is none
        out_pairs[v]  uint32  the outside pairs at v
        out_weight[v] uint32, out_node[v] int32  the greatest outside pair weight at v and the node at its other end, ties to the
                              smaller node; 0, -1 when there is none
        to_medoid[v]  uint32  the weight of the pair joining v and its cluster's medoid; 0 when there is none or v is the medoid

    Per cluster (EVALUATE_CLUSTER_ARRAYS), arrays of length n indexed by the naming node c = label[v] and read only where label[c] == c;
    0 or -1 elsewhere:

        size[c]   uint32  the members
        pairs[c], weight[c] uint64  the inside pairs and the sum of their weights
        min[c]    uint32  the weakest inside pair, 0xFFFFFFFF without one
        medoid[c] int32   the member of the greatest in_weight, ties to the smaller rank (greater score, then smaller index)
        near_weight[c] uint32, near_cluster[c] int32  the greatest weight of a pair joining a member and a non-member and the label of
                          the non-member, ties to the smaller label; 0, -1 without one

    Returns (the seven node arrays, the seven cluster arrays).  Integers, independent of the list's order, direction and duplication.
    More than 2^32 - 1 entries are refused: below that no 64-bit sum can overflow."""
    a, b, w, n = _check_entries(a, b, weight, n)
    if len(a) > EVALUATE_MAX_ENTRIES:
        raise ValueError(f"an evaluation is of at most {EVALUATE_MAX_ENTRIES} entries, not {len(a)}")
    label = check_partition(label, n)
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    if len(score) != n:
        raise ValueError(f"{n} nodes need {n} scores, not {len(score)}")
    _, rank = rank_order(score)
    # the distinct pairs (lo < hi) with the greatest weight of their entries: sorted by (lo, hi, weight), a run's last entry
    live = a != b
    lo, hi = np.minimum(a, b)[live], np.maximum(a, b)[live]
    w = np.ones(len(lo), dtype=np.uint64) if w is None else w[live].astype(np.uint64)
    if len(lo):
        by = np.lexsort((w, hi, lo))
        lo, hi, w = lo[by], hi[by], w[by]
        last = np.flatnonzero(np.append((lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1]), True))
        lo, hi, w = lo[last], hi[last], w[last]
    # every pair seen from both of its ends: v the node, o the other end
    v, o, wv = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    inside = label[v] == label[o]
    vi, oi, wi = v[inside], o[inside], wv[inside]
    vo, oo, wo = v[~inside], o[~inside], wv[~inside]
    low = np.uint64(0xFFFFFFFF)
    in_pairs = np.bincount(vi, minlength=n).astype(np.uint32)
    in_weight = _sum_by(vi, wi, n)
    in_min = np.full(n, EVALUATE_NONE, dtype=np.uint32)
    g, k = _pick_by(vi, wi, largest=False)
    in_min[g] = k.astype(np.uint32)
    out_pairs = np.bincount(vo, minlength=n).astype(np.uint32)
    out_weight, out_node = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    g, k = _pick_by(vo, (wo << np.uint64(32)) | (low - oo.astype(np.uint64)), largest=True)      # the greatest weight, then the smaller node
    out_weight[g], out_node[g] = (k >> np.uint64(32)).astype(np.uint32), (low - (k & low)).astype(np.int32)
    # per cluster: the naming nodes are those with label[c] == c
    names = label == np.arange(n)
    size = np.bincount(label, minlength=n).astype(np.uint32)
    once = lo[label[lo] == label[hi]]      # every inside pair once, by its lower end
    pairs = np.bincount(label[once], minlength=n).astype(np.uint64)
    weight_c = _sum_by(label[once], w[label[lo] == label[hi]], n)
    min_c = np.where(names, EVALUATE_NONE, 0).astype(np.uint32)
    g, k = _pick_by(label[vi], wi, largest=False)
    min_c[g] = k.astype(np.uint32)
    medoid = np.full(n, -1, dtype=np.int32)
    by = np.lexsort((rank, ~in_weight, label))      # by cluster, then in_weight descending (~ reverses uint64), then rank ascending
    first = np.flatnonzero(np.append(True, label[by][1:] != label[by][:-1]))
    medoid[label[by][first]] = by[first]
    near_weight, near_cluster = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    g, k = _pick_by(label[vo], (wo << np.uint64(32)) | (low - label[oo].astype(np.uint64)), largest=True)
    near_weight[g], near_cluster[g] = (k >> np.uint64(32)).astype(np.uint32), (low - (k & low)).astype(np.int32)
    to_medoid = np.zeros(n, dtype=np.uint32)
    hit = oi == medoid[label[vi]]
    to_medoid[vi[hit]] = wi[hit].astype(np.uint32)
    return ((in_pairs, in_weight, in_min, out_pairs, out_weight, out_node, to_medoid),
            (size, pairs, weight_c, min_c, medoid, near_weight, near_cluster))


class ScreenEvaluation(NamedTuple):
    """How good a partition of a list of kept pairs is, over the genomes `labels` (None: the nodes go by their index): label and score as
    they were given, then the seven node arrays and the seven cluster arrays of evaluate_of_pairs (the cluster arrays have length n and
    are indexed by the naming node).  Built by evaluation_from_nodes; clusters are numbered by ascending naming node."""
    labels: Optional[List[str]]
    label: np.ndarray            # int32[n]
    score: np.ndarray            # uint64[n]
    in_pairs: np.ndarray         # uint32[n]
    in_weight: np.ndarray        # uint64[n]
    in_min: np.ndarray           # uint32[n]
    out_pairs: np.ndarray        # uint32[n]
    out_weight: np.ndarray       # uint32[n]
    out_node: np.ndarray         # int32[n]
    to_medoid: np.ndarray        # uint32[n]
    size: np.ndarray             # uint32[n], by naming node, as the six below
    pairs: np.ndarray            # uint64[n]
    weight: np.ndarray           # uint64[n]
    min: np.ndarray              # uint32[n]
    medoid: np.ndarray           # int32[n]
    near_weight: np.ndarray      # uint32[n]
    near_cluster: np.ndarray     # int32[n]

    def node_arrays(self) -> tuple:
        return tuple(getattr(self, k) for k in EVALUATE_NODE_ARRAYS)

    def cluster_arrays(self) -> tuple:
        return tuple(getattr(self, k) for k in EVALUATE_CLUSTER_ARRAYS)

    def _names(self, nodes) -> list:
        """Labels of the nodes; "" for -1."""
        nodes = np.asarray(nodes).tolist()
        return [("" if i < 0 else (i if self.labels is None else self.labels[i])) for i in nodes]

    def naming(self) -> np.ndarray:
        """The naming nodes, ascending: cluster c of the frames is naming()[c]."""
        return np.flatnonzero(self.label == np.arange(len(self.label))).astype(np.int32)

    def cluster_of(self) -> np.ndarray:
        """int32[n]: the number of every node's cluster (the position of its label in naming())."""
        return np.searchsorted(self.naming(), self.label).astype(np.int32)

    def centrality(self) -> np.ndarray:
        """float64[n]: in_weight / (size - 1) of the node's cluster — the mean weight of a genome's pairs with the OTHER members of its
        cluster, an absent pair counting 0 (dRep's ANI 0); 0.0 in a singleton."""
        others = self.size[self.label].astype(np.float64) - 1.0
        return np.where(others > 0, self.in_weight.astype(np.float64) / np.where(others > 0, others, 1.0), 0.0)

    def complete(self) -> np.ndarray:
        """bool per cluster, in cluster order: every pair of members is a pair of the list (pairs == size (size - 1) / 2)."""
        s = self.size[self.naming()].astype(np.uint64)
        return self.pairs[self.naming()] == s * (s - np.uint64(1)) // np.uint64(2)

    def genome_frame(self) -> pd.DataFrame:
        """One row per genome, in the order of `labels`: genome, cluster, medoid (of its cluster), is_medoid, centrality, in_pairs,
        in_weight, in_min, to_medoid, out_pairs, out_weight, out_node ("" when there is none)."""
        n = len(self.label)
        med = self.medoid[self.label]
        return pd.DataFrame({"genome": self._names(np.arange(n)), "cluster": self.cluster_of().astype(np.int64), "medoid": self._names(med),
                             "is_medoid": med == np.arange(n), "centrality": self.centrality(), "in_pairs": self.in_pairs.astype(np.int64),
                             "in_weight": self.in_weight, "in_min": self.in_min.astype(np.int64), "to_medoid": self.to_medoid.astype(np.int64),
                             "out_pairs": self.out_pairs.astype(np.int64), "out_weight": self.out_weight.astype(np.int64), "out_node": self._names(self.out_node)})

    def cluster_frame(self) -> pd.DataFrame:
        """One row per cluster, by ascending naming node: cluster, name (the naming node), size, pairs, complete, weight, mean_weight
        (weight / pairs, 0.0 without a pair), min, medoid, near_weight, near_cluster (a cluster number, -1 when there is none)."""
        c = self.naming()
        pairs = self.pairs[c]
        mean = np.where(pairs > 0, self.weight[c].astype(np.float64) / np.where(pairs > 0, pairs, 1).astype(np.float64), 0.0)
        near = self.near_cluster[c]
        near_no = np.where(near >= 0, np.searchsorted(c, np.maximum(near, 0)), -1).astype(np.int64)
        return pd.DataFrame({"cluster": np.arange(len(c), dtype=np.int64), "name": self._names(c), "size": self.size[c].astype(np.int64), "pairs": pairs,
                             "complete": self.complete(), "weight": self.weight[c], "mean_weight": mean, "min": self.min[c].astype(np.int64),
                             "medoid": self._names(self.medoid[c]), "near_weight": self.near_weight[c].astype(np.int64), "near_cluster": near_no})

    def proximity(self, min_weight: int = 0) -> pd.DataFrame:
        """The "these two nearly merge" table: one row per cluster that has an outside pair of weight near_weight >= min_weight —
        cluster, name, near_cluster, near_name, near_weight, in cluster order.  A cluster without an outside pair has no row."""
        t = self.cluster_frame()
        keep = ((t["near_cluster"] >= 0) & (t["near_weight"] >= int(min_weight))).to_numpy()
        t = t[keep].reset_index(drop=True)
        names = self._names(self.naming())
        return pd.DataFrame({"cluster": t["cluster"], "name": t["name"], "near_cluster": t["near_cluster"],
                             "near_name": [names[i] for i in t["near_cluster"].tolist()], "near_weight": t["near_weight"]})

    def recentred(self) -> "ScreenClusters":
        """The same clusters with every cluster's MEDOID as its representative: rep[v] = medoid[label[v]], via = to_medoid."""
        return clusters_from_nodes(self.labels, self.medoid[self.label], self.to_medoid, self.score)


def evaluation_from_nodes(labels, label, score, node_arrays, cluster_arrays) -> ScreenEvaluation:
    """The ScreenEvaluation of what evaluate_of_pairs or Engine.screen_evaluate returned."""
    score = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
    n = len(score)
    label = check_partition(label, n).astype(np.int32)
    if labels is not None:
        labels = [str(x) for x in labels]
        if len(labels) != n:
            raise ValueError("labels and nodes must have the same length")
    if len(node_arrays) != len(EVALUATE_NODE_ARRAYS) or len(cluster_arrays) != len(EVALUATE_CLUSTER_ARRAYS):
        raise ValueError(f"an evaluation has {len(EVALUATE_NODE_ARRAYS)} node arrays and {len(EVALUATE_CLUSTER_ARRAYS)} cluster arrays")
    nodes = [np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(node_arrays, _EVALUATE_NODE_TYPES)]
    clusters = [np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(cluster_arrays, _EVALUATE_CLUSTER_TYPES)]
    if any(len(x) != n for x in nodes + clusters):
        raise ValueError("every array of an evaluation has one entry per node")
    medoid = clusters[4]
    names = label == np.arange(n)
    if n and ((medoid[names] < 0).any() or (medoid[names] >= n).any() or (label[medoid[names]] != np.flatnonzero(names)).any()):
        raise ValueError("a cluster's medoid is no member of it")
    return ScreenEvaluation(labels, label, score, *nodes, *clusters)


# ---- the profile of a partition over the search index ----------------------------------------------------------------------
PROFILE_GENOME_ARRAYS = ("held", "core_held", "private_held", "alone", "foreign")
PROFILE_CLUSTER_ARRAYS = ("size", "kmers", "core", "soft", "shell", "private", "marker")
PROFILE_MARKER_ARRAYS = ("marker_cluster", "marker_kmer", "marker_occ")
_PROFILE_GENOME_TYPES = (np.uint32,) * 5
_PROFILE_CLUSTER_TYPES = (np.uint32,) + (np.uint64,) * 6
_PROFILE_MARKER_TYPES = (np.int32, np.uint32, np.uint32)
PROFILE_LANE_MAX, PROFILE_WAVE_MAX = 8, 64      # Engine.screen_search_profile_set: the largest settable tier limits


def profile_thresholds(size, core: float = 0.95, shell: float = 0.15) -> Tuple[np.ndarray, np.ndarray]:
    """(core_need, shell_need) uint32 per entry of `size`: max(1, ceil(fraction * size)), computed exactly from the rational value of the
    float (fractions.Fraction), never in floating point; 0 where size is 0 (a node that names no cluster).  ValueError unless
    0 < shell <= core <= 1."""
    from fractions import Fraction
    try:
        ok = 0 < shell <= core <= 1
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"the profile's fractions must satisfy 0 < shell <= core <= 1, not shell={shell!r}, core={core!r}")
    size = np.ascontiguousarray(size, dtype=np.int64).reshape(-1)
    if (size < 0).any():
        raise ValueError("a cluster's size is not negative")
    distinct, where = np.unique(size, return_inverse=True)
    out = []
    for fraction in (Fraction(core), Fraction(shell)):
        p, q = fraction.numerator, fraction.denominator
        need = [max(1, -((-p * s) // q)) if s else 0 for s in distinct.tolist()]      # (Python integers: exact at any size)
        out.append(np.array(need, dtype=np.uint32)[where.reshape(-1)])
    return out[0], out[1]


def check_profile_thresholds(label, core_need, shell_need) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(size, core_need, shell_need) uint32[n] of a partition (check_partition) with its thresholds: size[c] the members of the cluster that
    node c names, 0 elsewhere; ValueError names the first naming node with other than 1 <= shell_need <= core_need <= size."""
    n = len(label)
    size = np.bincount(label, minlength=n).astype(np.uint32)
    try:
        need = [np.ascontiguousarray(x).reshape(-1) for x in (core_need, shell_need)]
    except (TypeError, ValueError) as err:
        raise ValueError(f"thresholds must be integers: {err}") from None
    if any(len(x) != n for x in need) or any(x.dtype.kind not in "iu" for x in need):
        raise ValueError(f"{n} nodes need {n} integer core_need and shell_need each")
    c64, s64 = (x.astype(np.int64) for x in need)
    bad = (size > 0) & ((s64 < 1) | (s64 > c64) | (c64 > size))
    if bad.any():
        c = int(np.flatnonzero(bad)[0])
        raise ValueError(f"node {c} names a cluster of {int(size[c])} with the thresholds {int(s64[c])} and {int(c64[c])} (1 <= shell_need <= core_need <= size)")
    names = size > 0
    return size, np.where(names, c64, 0).astype(np.uint32), np.where(names, s64, 0).astype(np.uint32)


def profile_of_index(kmer, start, member, n, label, core_need, shell_need, marker_min_size: int = 2):
    """THE STATEMENT of the profile (the host's; Engine.screen_search_profile is held to it), over the arrays of an exported search index
    (kmer uint32[D], start uint64[D + 1], member uint32[E]: k-mer d is held by H(d) = member[start[d]:start[d + 1]], h(d) = |H(d)| >= 1), a
    partition label (check_partition) and two thresholds per naming node, 1 <= shell_need[c] <= core_need[c] <= size[c].

    A CELL is a pair (d, c) with occ = |H(d) & c| > 0.  It is core iff occ == size[c], soft iff occ >= core_need[c], shell iff
    shell_need[c] <= occ < core_need[c], private iff occ == h(d), a marker iff private and soft.  Returns (genome arrays, cluster arrays,
    spectrum, off, marker arrays):

        per genome v of cluster c, uint32[n] (PROFILE_GENOME_ARRAYS): held = its k-mers; core_held = those whose cell in c is soft;
            private_held = those whose cell in c is private; alone = those with occ == 1; foreign = those of alone with h(d) > 1
        per cluster, length n by naming node, 0 elsewhere (PROFILE_CLUSTER_ARRAYS): size uint32; kmers, core, soft, shell, private, marker
            uint64, its cells of each kind (kmers: all)
        spectrum uint64[n], off int64[n]: off[c] = the members of the clusters with a smaller naming node (0 where c names none);
            spectrum[off[c] + occ - 1] = the cells of c with that occ
        markers (PROFILE_MARKER_ARRAYS): the marker cells of the clusters with size >= marker_min_size as (cluster int32, the k-mer's
            value uint32, occ uint32), by ascending cluster, then by the k-mer's position in the index

    One lexsort of the entries by (k-mer position, cluster), then runs.  Integers only."""
    n = int(n)
    label = check_partition(label, n)
    size, core_need, shell_need = check_profile_thresholds(label, core_need, shell_need)
    if isinstance(marker_min_size, (bool, float)) or int(marker_min_size) < 1:
        raise ValueError(f"marker_min_size is an integer >= 1, not {marker_min_size!r}")
    kmer = np.ascontiguousarray(kmer, dtype=np.uint32).reshape(-1)
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1).astype(np.int64)
    member = np.ascontiguousarray(member, dtype=np.uint32).reshape(-1).astype(np.int64)
    d, e = len(kmer), len(member)
    if len(start) != d + 1 or start[0] != 0 or start[-1] != e or (np.diff(start) < 1).any() or (e and member.max() >= n):
        raise ValueError("the arrays are not those of a search index over n genomes")
    names = size > 0
    off = np.where(names, np.cumsum(np.where(names, size, 0).astype(np.int64)) - size, 0).astype(np.int64)
    h = np.diff(start)
    pos = np.repeat(np.arange(d, dtype=np.int64), h)              # the k-mer of every entry
    cl = label[member]
    by = np.lexsort((cl, pos))
    pos_s, cl_s, mem_s = pos[by], cl[by], member[by]
    head = np.ones(e, dtype=bool)
    head[1:] = (pos_s[1:] != pos_s[:-1]) | (cl_s[1:] != cl_s[:-1])
    first = np.flatnonzero(head)
    occ = np.diff(np.append(first, e))                            # per cell
    cd, cc = pos_s[first], cl_s[first]
    ch = h[cd]
    core = occ == size[cc]
    soft = occ >= core_need[cc]
    shell = ~soft & (occ >= shell_need[cc])
    private = occ == ch
    marker = private & soft

    def per_cluster(mask):
        return np.bincount(cc[mask], minlength=n).astype(np.uint64)

    every = np.ones(len(cc), dtype=bool)
    clusters = (size, per_cluster(every), per_cluster(core), per_cluster(soft), per_cluster(shell), per_cluster(private), per_cluster(marker))
    spectrum = np.bincount(off[cc] + occ - 1, minlength=n).astype(np.uint64)
    cell = np.cumsum(head) - 1                                    # the cell of every sorted entry
    e_occ, e_h = occ[cell], ch[cell]

    def per_genome(mask):
        return np.bincount(mem_s[mask], minlength=n).astype(np.uint32)

    genomes = (per_genome(np.ones(e, dtype=bool)), per_genome(soft[cell]), per_genome(private[cell]), per_genome(e_occ == 1), per_genome((e_occ == 1) & (e_h > 1)))
    listed = np.flatnonzero(marker & (size[cc] >= int(marker_min_size)))
    listed = listed[np.lexsort((cd[listed], cc[listed]))]
    markers = (cc[listed].astype(np.int32), kmer[cd[listed]], occ[listed].astype(np.uint32))
    return genomes, clusters, spectrum, off, markers


_KMER_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def kmer_string(value, k: int) -> str:
    """The canonical k-mer `value` as ACGT text in the scan's own 2-bit code: A, C, G, T = 0, 1, 2, 3, the first base in the high bits of
    the 2 k bit word."""
    k, value = int(k), int(value)
    if not 1 <= k <= 16 or not 0 <= value < 4 ** k:
        raise ValueError(f"a {k}-mer's value is below 4^{k} (k <= 16), not {value}")
    return "".join("ACGT"[(value >> (2 * (k - 1 - i))) & 3] for i in range(k))


class ScreenProfile(NamedTuple):
    """What the genomes of every cluster share, over the genomes `labels` (None: the nodes go by their index): the partition and its
    thresholds as they were given, then the arrays of profile_of_index.  Built by profile_from_arrays; clusters are numbered by ascending
    naming node.  Every count is of SAMPLED k-mers: at scale s it estimates 1 / s of the count over all k-mers (scale 1: all of them)."""
    labels: Optional[List[str]]
    kmer: int                      # the index's k, for markers_frame's text (0: unknown, values are printed as numbers)
    label: np.ndarray              # int32[n]
    core_need: np.ndarray          # uint32[n], by naming node, 0 elsewhere
    shell_need: np.ndarray         # uint32[n]
    marker_min_size: int
    held: np.ndarray               # uint32[n]
    core_held: np.ndarray          # uint32[n]
    private_held: np.ndarray       # uint32[n]
    alone: np.ndarray              # uint32[n]
    foreign: np.ndarray            # uint32[n]
    size: np.ndarray               # uint32[n], by naming node, as the six below
    kmers: np.ndarray              # uint64[n]
    core: np.ndarray               # uint64[n]
    soft: np.ndarray               # uint64[n]
    shell: np.ndarray              # uint64[n]
    private: np.ndarray            # uint64[n]
    marker: np.ndarray             # uint64[n]
    spectrum: np.ndarray           # uint64[n]
    off: np.ndarray                # int64[n]: the first spectrum word of the cluster a node names
    marker_cluster: np.ndarray     # int32[m]: naming nodes
    marker_kmer: np.ndarray        # uint32[m]
    marker_occ: np.ndarray         # uint32[m]

    def genome_arrays(self) -> tuple:
        return tuple(getattr(self, k) for k in PROFILE_GENOME_ARRAYS)

    def cluster_arrays(self) -> tuple:
        return tuple(getattr(self, k) for k in PROFILE_CLUSTER_ARRAYS)

    def marker_arrays(self) -> tuple:
        return tuple(getattr(self, k) for k in PROFILE_MARKER_ARRAYS)

    def _names(self, nodes) -> list:
        nodes = np.asarray(nodes).tolist()
        return [(i if self.labels is None else self.labels[i]) for i in nodes]

    def naming(self) -> np.ndarray:
        """The naming nodes, ascending: cluster c of the frames is naming()[c]."""
        return np.flatnonzero(self.label == np.arange(len(self.label))).astype(np.int32)

    def cluster_of(self) -> np.ndarray:
        """int32[n]: the number of every node's cluster (the position of its label in naming())."""
        return np.searchsorted(self.naming(), self.label).astype(np.int32)

    def spectrum_of(self, c) -> np.ndarray:
        """uint64[size]: entry occ - 1 = the cells of the cluster that node c names with that occupancy."""
        c = int(c)
        if not 0 <= c < len(self.label) or int(self.label[c]) != c:
            raise ValueError(f"node {c} names no cluster")
        return self.spectrum[int(self.off[c]):int(self.off[c]) + int(self.size[c])]

    def genome_frame(self) -> pd.DataFrame:
        """One row per genome, in the order of `labels`: genome, cluster, held, core_held, core_missing (soft of its cluster - core_held),
        core_fraction (core_held / soft, NaN when soft is 0), private_held, alone, foreign, singleton (alone - foreign)."""
        n = len(self.label)
        soft = self.soft[self.label].astype(np.int64)
        core_held = self.core_held.astype(np.int64)
        fraction = np.where(soft > 0, core_held.astype(np.float64) / np.where(soft > 0, soft, 1).astype(np.float64), np.nan)
        return pd.DataFrame({"genome": self._names(np.arange(n)), "cluster": self.cluster_of().astype(np.int64), "held": self.held.astype(np.int64),
                             "core_held": core_held, "core_missing": soft - core_held, "core_fraction": fraction,
                             "private_held": self.private_held.astype(np.int64), "alone": self.alone.astype(np.int64), "foreign": self.foreign.astype(np.int64),
                             "singleton": self.alone.astype(np.int64) - self.foreign.astype(np.int64)})

    def cluster_frame(self) -> pd.DataFrame:
        """One row per cluster, by ascending naming node: cluster, name (the naming node), size, core_need, shell_need, kmers, core, soft,
        shell, cloud (kmers - soft - shell), private, marker."""
        c = self.naming()
        cols = {"cluster": np.arange(len(c), dtype=np.int64), "name": self._names(c), "size": self.size[c].astype(np.int64),
                "core_need": self.core_need[c].astype(np.int64), "shell_need": self.shell_need[c].astype(np.int64)}
        for k in ("kmers", "core", "soft", "shell"):
            cols[k] = getattr(self, k)[c].astype(np.int64)
        cols["cloud"] = cols["kmers"] - cols["soft"] - cols["shell"]
        cols["private"], cols["marker"] = self.private[c].astype(np.int64), self.marker[c].astype(np.int64)
        return pd.DataFrame(cols)

    def spectrum_frame(self) -> pd.DataFrame:
        """cluster, occupancy, kmers: the spectrum without its zero rows, by cluster, then occupancy."""
        c = self.naming()
        number = np.repeat(np.arange(len(c), dtype=np.int64), self.size[c].astype(np.int64))      # (the spectrum's words stand in this order)
        occupancy = np.arange(len(self.spectrum), dtype=np.int64) - np.repeat(self.off[c], self.size[c].astype(np.int64)) + 1
        keep = self.spectrum > 0
        return pd.DataFrame({"cluster": number[keep], "occupancy": occupancy[keep], "kmers": self.spectrum[keep].astype(np.int64)})

    def markers_frame(self) -> pd.DataFrame:
        """One row per listed marker, in the list's order: cluster (its number), name, kmer (ACGT text when the index's k is known),
        occupancy."""
        text = [kmer_string(x, self.kmer) for x in self.marker_kmer.tolist()] if self.kmer else self.marker_kmer.astype(np.int64)
        return pd.DataFrame({"cluster": np.searchsorted(self.naming(), self.marker_cluster).astype(np.int64), "name": self._names(self.marker_cluster),
                             "kmer": text, "occupancy": self.marker_occ.astype(np.int64)})


def profile_from_arrays(labels, label, core_need, shell_need, marker_min_size, genome_arrays, cluster_arrays, spectrum, marker_arrays, kmer: int = 0) -> ScreenProfile:
    """The ScreenProfile of what profile_of_index or Engine.screen_search_profile returned (off is computed from the sizes)."""
    label = np.ascontiguousarray(label, dtype=np.int64).reshape(-1)
    n = len(label)
    label = check_partition(label, n)
    if labels is not None:
        labels = [str(x) for x in labels]
        if len(labels) != n:
            raise ValueError("labels and nodes must have the same length")
    if len(genome_arrays) != len(PROFILE_GENOME_ARRAYS) or len(cluster_arrays) != len(PROFILE_CLUSTER_ARRAYS) or len(marker_arrays) != len(PROFILE_MARKER_ARRAYS):
        raise ValueError(f"a profile has {len(PROFILE_GENOME_ARRAYS)} genome arrays, {len(PROFILE_CLUSTER_ARRAYS)} cluster arrays and {len(PROFILE_MARKER_ARRAYS)} marker arrays")
    genomes = [np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(genome_arrays, _PROFILE_GENOME_TYPES)]
    clusters = [np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(cluster_arrays, _PROFILE_CLUSTER_TYPES)]
    markers = [np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(marker_arrays, _PROFILE_MARKER_TYPES)]
    spectrum = np.ascontiguousarray(spectrum, dtype=np.uint64).reshape(-1)
    if any(len(x) != n for x in genomes + clusters + [spectrum]) or len({len(x) for x in markers}) != 1:
        raise ValueError("every array of a profile has one entry per node, and the markers' columns one length")
    size = clusters[0]
    if not np.array_equal(size, np.bincount(label, minlength=n)):
        raise ValueError("the sizes are not those of the partition")
    _, core_need, shell_need = check_profile_thresholds(label, core_need, shell_need)
    names = size > 0
    off = np.where(names, np.cumsum(np.where(names, size, 0).astype(np.int64)) - size, 0).astype(np.int64)
    return ScreenProfile(labels, int(kmer), label.astype(np.int32), core_need, shell_need, int(marker_min_size), *genomes, *clusters, spectrum, off, *markers)


def _labels_for(ids, labels, limit: int = MAX_GENOMES) -> List[str]:
    labels = [str(x) for x in (ids if labels is None else labels)]
    if len(labels) != len(ids):
        raise ValueError("ids and labels must have the same length")
    if len(ids) > limit:
        raise ValueError(f"a screen call takes at most {limit} genomes, not {len(ids)}")
    return labels


def index_candidates_on(engines, run_all, ids, options, labels=None) -> ScreenedPairs:
    """The selection through the index on the D engines given: every one builds the index of `ids` (the genome store is
    replicated, and so is this scan), engine d selects the bands d, d + D, ..., and the parts are merged by merge_dealt; the indexes are
    released, on errors too.  run_all(fn) -> [fn(engine, d) for each engine] (in threads for several).  Equal to the dense path."""
    options = check_options(options)
    ids = list(ids)
    labels = _labels_for(ids, labels, INDEX_MAX_GENOMES)
    if not ids:
        return ScreenedPairs(labels, options, np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    d = len(engines)

    def part(engine, k):
        sizes = engine.screen_index(ids, options.kmer, options.scale)
        need = identity_thresholds(sizes, options.kmer, options.min_identity, options.min_shared)
        return sizes, engine.screen_index_select(need, band_first=k, band_step=d)
    try:
        parts = run_all(part)
    finally:
        for e in engines:
            e.screen_index_release()
    a, b, shared = parts[0][1] if d == 1 else merge_dealt([p[1] for p in parts])
    return ScreenedPairs(labels, options, parts[0][0], a, b, shared)


def candidates_on(engine, make_resident, ids, options, labels=None) -> ScreenedPairs:
    """The selection on one Engine: make_resident() leaves the matrix of `ids` on it and returns the sizes; then thresholds, select,
    release (on errors too).  Engine.screen_candidates and MultiEngine.screen_candidates are this with their own make_resident."""
    options = check_options(options)
    ids = list(ids)
    labels = _labels_for(ids, labels)
    if not ids:
        return ScreenedPairs(labels, options, np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    try:
        sizes = make_resident()
        need = identity_thresholds(sizes, options.kmer, options.min_identity, options.min_shared)
        a, b, shared = engine.screen_select(need)
    finally:
        engine.screen_release()
    return ScreenedPairs(labels, options, sizes, a, b, shared)


class ScreenResult(NamedTuple):
    labels: List[str]
    kmer: int
    scale: int
    sizes: np.ndarray       # uint32[n]
    shared: np.ndarray      # uint32[n, n], symmetric, the diagonal = sizes

    def _frame(self, values) -> pd.DataFrame:
        return pd.DataFrame(values, index=list(self.labels), columns=list(self.labels))

    def _containment(self) -> np.ndarray:
        size = self.sizes.astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(size > 0, self.shared.astype(np.float64) / size, np.nan)

    def shared_frame(self) -> pd.DataFrame:
        return self._frame(self.shared)

    def containment(self) -> pd.DataFrame:
        """shared[a][b] / sizes[a]: the share of genome a's sampled k-mers found in genome b; NaN on the rows of empty genomes."""
        return self._frame(self._containment())

    def jaccard(self) -> pd.DataFrame:
        s = self.sizes.astype(np.float64)
        sh = self.shared.astype(np.float64)
        union = s[:, None] + s[None, :] - sh
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._frame(np.where(union > 0, sh / union, np.nan))

    def _identity(self, min_shared: int) -> np.ndarray:
        c = self._containment()
        ok = self.shared >= int(min_shared)
        return np.where(ok, np.power(np.where(ok, c, 1.0), 1.0 / self.kmer), 0.0)

    def identity(self, min_shared: int = DEFAULT_MIN_SHARED) -> pd.DataFrame:
        """containment ** (1 / k) where at least min_shared k-mers are shared, else 0.0 (so an empty genome's row is 0.0 for every
        min_shared >= 1, and NaN as its containment is for min_shared = 0)."""
        return self._frame(self._identity(min_shared))

    def candidate_pairs(self, min_identity: float, min_shared: int = DEFAULT_MIN_SHARED) -> List[Tuple[int, int]]:
        """The ordered pairs (a, b) and (b, a), as positions in `labels`, of every a != b with
        max(identity[a][b], identity[b][a]) >= min_identity, in row-major order: ready for anim_pairs / anib_pairs."""
        ident = self._identity(min_shared)
        keep = np.maximum(ident, ident.T) >= float(min_identity)
        np.fill_diagonal(keep, False)
        a, b = np.nonzero(keep)
        return list(zip(a.tolist(), b.tolist()))


def screen_genomes(engine, ids: Sequence[int], labels: Sequence[str], kmer: int = DEFAULT_KMER, scale: int = DEFAULT_SCALE) -> ScreenResult:
    """The screen of the resident genomes `ids` (an Engine or a MultiEngine), labelled in that order."""
    kmer, scale = check_params(kmer, scale)
    ids, labels = list(ids), [str(x) for x in labels]
    if len(ids) != len(labels):
        raise ValueError("ids and labels must have the same length")
    if len(set(labels)) != len(labels):
        raise ValueError("two genomes share a label")
    if len(ids) > MAX_GENOMES:
        raise ValueError(f"a screen call takes at most {MAX_GENOMES} genomes, not {len(ids)}")
    sizes, shared = engine.screen_matrix(ids, kmer=kmer, scale=scale)
    return ScreenResult(labels, kmer, scale, sizes, shared)


# ---- the search: new genomes against a resident collection ------------------------------------------------------------------
def select_rectangle(hits, need_q, need_db) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """THE STATEMENT of the search's selection (the host's; Engine.screen_search_select is held to it): for hits uint32[q, n] — hits[i][b] =
    the sampled k-mers query i shares with db genome b — the triples (i, b, hits[i][b]) with hits[i][b] >= min(need_q[i], need_db[b]),
    row-major: int32, int32, uint32.  The rule of candidate_pairs (identity_thresholds) on a rectangle; there is no diagonal: a query
    that is also a db genome meets itself like any other."""
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    need_q = np.ascontiguousarray(need_q, dtype=np.uint32).reshape(-1)
    need_db = np.ascontiguousarray(need_db, dtype=np.uint32).reshape(-1)
    if hits.ndim != 2 or hits.shape != (len(need_q), len(need_db)):
        raise ValueError(f"hits of shape {hits.shape} do not go with {len(need_q)} query and {len(need_db)} db thresholds")
    a, b = np.nonzero(hits >= np.minimum.outer(need_q, need_db))
    return a.astype(np.int32), b.astype(np.int32), hits[a, b]


def merge_search_parts(parts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, shared) of a search whose collection was dealt into contiguous ranges of columns: parts[d] = (col0, a, b, shared), the
    row-major triples of ALL queries against the db genomes [col0, col0 + n_d), b counted from col0; the ranges ascend with d.  The column
    offsets are added and the parts merged per query row in ascending d (a stable sort on the row): ascending b inside a row follows."""
    a = np.concatenate([np.asarray(p[1], dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    b = np.concatenate([np.asarray(p[2], dtype=np.int32) + np.int32(p[0]) for p in parts]) if parts else np.zeros(0, np.int32)
    s = np.concatenate([np.asarray(p[3], dtype=np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32)
    order = np.argsort(a, kind="stable")
    return a[order], b[order], s[order]


def merge_search_index(kmer, start, member, new_kmer, new_member):
    """THE STATEMENT of the search index's growth (the device's steps 3 to 5) on arrays, for an index of ONE slice: the
    index (kmer uint32[D] ascending, start int64[D + 1], member uint32[E], ascending inside a k-mer) and the entries of the added genomes
    (new_kmer, new_member, sorted by k-mer, then member; every new member larger than every old one) -> (kmer', start', member', new
    k-mers, matched k-mers).  An added k-mer is looked up (lower bound p); an absent one is ranked among the absent (a) and goes to p + a,
    an old k-mer g moves up by the absent ones with p <= g, and the new entries go behind their k-mer's old holders — nothing is sorted."""
    kmer, start, member = np.asarray(kmer, dtype=np.uint32), np.asarray(start, dtype=np.int64), np.asarray(member, dtype=np.uint32)
    new_kmer, new_member = np.asarray(new_kmer, dtype=np.uint32), np.asarray(new_member, dtype=np.uint32)
    d, e, nk = len(kmer), len(member), len(new_kmer)
    old_count = np.diff(start)
    head = np.ones(nk, dtype=bool)
    head[1:] = new_kmer[1:] != new_kmer[:-1]
    run_first = np.flatnonzero(head)
    run_len = np.diff(np.append(run_first, nk))
    canon = new_kmer[run_first]
    p = np.searchsorted(kmer, canon, side="left")
    found = np.zeros(len(canon), dtype=bool)
    inside = p < d
    found[inside] = kmer[p[inside]] == canon[inside]
    absent = ~found
    a = np.cumsum(absent) - absent                                        # the absent runs before each run
    shift = np.cumsum(np.bincount(p[absent], minlength=d + 1))[:d]        # the absent runs that go before each old k-mer
    d_new = d + int(absent.sum())
    old_pos, run_pos = np.arange(d) + shift, p + a
    kmer_new, count = np.zeros(d_new, dtype=np.uint32), np.zeros(d_new, dtype=np.int64)
    kmer_new[old_pos], count[old_pos] = kmer, old_count
    kmer_new[run_pos[absent]] = canon[absent]
    count[run_pos] += run_len
    start_new = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    member_new = np.zeros(e + nk, dtype=np.uint32)
    of_entry = np.repeat(np.arange(d), old_count)
    member_new[np.arange(e) + (start_new[old_pos] - start[:d])[of_entry]] = member
    behind = np.zeros(len(canon), dtype=np.int64)
    behind[found] = old_count[p[found]]
    of_key = np.repeat(np.arange(len(canon)), run_len)
    member_new[(start_new[run_pos] + behind)[of_key] + np.arange(nk) - run_first[of_key]] = new_member
    return kmer_new, start_new, member_new, int(absent.sum()), int(found.sum())


def remove_from_search_index(kmer, start, member, n, columns):
    """THE STATEMENT of the search index's shrinking on arrays, for an index of ONE slice: the index of n genomes (kmer
    uint32[D] ascending, start int64[D + 1], member uint32[E], ascending inside a k-mer) without the columns `columns` (each < n, none
    twice) -> (kmer', start', member', removed entries, removed k-mers).  A surviving column c becomes c - (removed columns below c);
    the surviving entries keep their order, a k-mer whose last holder went is dropped — nothing is sorted."""
    kmer, start, member = np.asarray(kmer, dtype=np.uint32), np.asarray(start, dtype=np.int64), np.asarray(member, dtype=np.uint32)
    columns = np.asarray(columns, dtype=np.int64).reshape(-1)
    n = int(n)
    if len(columns) and (columns.min() < 0 or columns.max() >= n):
        raise ValueError(f"a column to remove is not in an index of {n} genomes")
    if len(np.unique(columns)) != len(columns):
        raise ValueError("a column to remove is given twice")
    keep = np.ones(n, dtype=bool)
    keep[columns] = False
    new_of = np.cumsum(keep) - keep                                      # the kept columns below each column
    alive = keep[member] if len(member) else np.zeros(0, dtype=bool)
    pos = np.concatenate([[0], np.cumsum(alive)]).astype(np.int64)       # the entries' new positions; pos[E] = E'
    count = pos[start[1:]] - pos[start[:-1]]                             # the holders each k-mer keeps
    kept = count > 0
    start_new = np.concatenate([pos[start[:-1]][kept], pos[-1:]]).astype(np.int64)
    member_new = new_of[member[alive]].astype(np.uint32)
    return kmer[kept], start_new, member_new, int(len(member) - len(member_new)), int(len(kmer) - int(kept.sum()))


# ---- the search index on disk -------------------------------------------------------------------------------------------
N_BINS = 4096                       # pgscr::N_BINS: the slice bins of a sampled k-mer
SEARCH_NO_SLICE = 0xFFFFFFFF        # bin_slice of a bin that no slice covers


def mix32(h) -> np.ndarray:
    """pgs::mix32 (pg_sketch_core.h) on uint32 arrays: murmur3's finaliser."""
    h = np.array(h, dtype=np.uint32, copy=True).reshape(-1)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def log2_scale(scale: int) -> int:
    return int(scale).bit_length() - 1


def kmer_sampled(canon, scale: int) -> np.ndarray:
    """pgs::sampled: the FracMinHash rule, mix32(canon) & (scale - 1) == 0."""
    return (mix32(canon) & np.uint32(int(scale) - 1)) == 0


def kmer_bin(canon, scale: int) -> np.ndarray:
    """pgscr::bin_of (pg_screen_core.h): (mix32(canon) >> log2(scale)) & 4095, the hash bits above the ones the sampling reads."""
    return (mix32(canon) >> np.uint32(log2_scale(scale))) & np.uint32(N_BINS - 1)


SEARCH_INDEX_INVARIANTS = {
    "shape": "the shape is out of range (n <= 2^20, 8 <= kmer <= 16, scale a power of two <= 65536, E >= D, slices <= 4096, n = 0 with D = E = 0)",
    "lengths": "an array has not the length its shape gives",
    "slice_first": "slice_first does not begin at 0, ascend and end at D",
    "bin_slice": "a bin names a slice that is not there",
    "start0": "start[0] is not 0",
    "start_end": "start[D] is not E",
    "start_order": "start is not strictly increasing",
    "kmer_range": "k-mers are not below 4^kmer",
    "kmer_sampled": "k-mers are not sampled under the scale",
    "kmer_slice": "k-mers stand outside the slice of their bin",
    "kmer_order": "k-mers are not strictly ascending inside a slice",
    "member_range": "members are not below n",
    "member_order": "members are not strictly ascending inside a k-mer",
}


def check_search_index(shape, kmer, start, member, slice_first, bin_slice) -> List[str]:
    """THE STATEMENT of the import's validation (pg_screen_search_index_import): the texts (values of SEARCH_INDEX_INVARIANTS, each followed
    by its count where it has one) of EVERY invariant of a built search index that the arrays violate; [] for a sound index.  shape = (n,
    kmer, scale, D, E, n_slices, keys).  As on the device nothing is indexed by a value that was not checked first: a violated host check
    ends the list, and the entries are walked only when the starts are sound."""
    inv = SEARCH_INDEX_INVARIANTS
    n, k, scale, d, e, s = (int(x) for x in list(shape)[:6])
    kmer, member, bin_slice = (np.asarray(x, dtype=np.uint32).reshape(-1) for x in (kmer, member, bin_slice))
    start, slice_first = (np.asarray(x, dtype=np.uint64).reshape(-1) for x in (start, slice_first))
    if n > INDEX_MAX_GENOMES or not 8 <= k <= 16 or not (1 <= scale <= 65536 and scale & (scale - 1) == 0) or e < d or s > N_BINS or (n == 0 and (d or e)):
        return [inv["shape"]]
    if (len(kmer), len(start), len(member), len(slice_first), len(bin_slice)) != (d, d + 1, e, s + 1, N_BINS):
        return [inv["lengths"]]
    if n == 0:
        return []
    host = []
    if slice_first[0] != 0 or (np.diff(slice_first.astype(np.int64)) < 0).any() or slice_first[s] != d:
        host.append(inv["slice_first"])
    if ((bin_slice >= s) & (bin_slice != SEARCH_NO_SLICE)).any():
        host.append(inv["bin_slice"])
    if host:
        return host
    out = []

    def count(name, bad):
        c = int(np.count_nonzero(bad))
        if c:
            out.append(f"{inv[name]} ({c} of them)")

    count("start0", start[:1] != 0)
    count("start_end", start[d:] != e)
    order = ~(start[:-1] < start[1:])
    count("start_order", order)
    count("kmer_range", kmer.astype(np.uint64) >= (np.uint64(1) << np.uint64(2 * k)))
    count("kmer_sampled", ~kmer_sampled(kmer, scale))
    g = np.arange(d, dtype=np.uint64)
    of = np.searchsorted(slice_first[:s], g, side="right").astype(np.int64) - 1      # the last slice that begins at or before g
    count("kmer_slice", bin_slice[kmer_bin(kmer, scale)].astype(np.int64) != of)
    if d:
        first_of_slice = g == slice_first[of]
        count("kmer_order", ~first_of_slice[1:] & (kmer[:-1] >= kmer[1:]))
    if start[0] == 0 and start[d] == e and not order.any() and e:
        count("member_range", member >= n)
        first_of_kmer = np.zeros(e, dtype=bool)
        first_of_kmer[start[:-1].astype(np.int64)] = True
        count("member_order", ~first_of_kmer[1:] & (member[:-1] >= member[1:]))
    return out


def search_index_sizes(member, n: int) -> np.ndarray:
    """sizes uint32[n] of an index's genomes: the entries per column, as the import computes them."""
    return np.bincount(np.asarray(member, dtype=np.int64), minlength=int(n)).astype(np.uint32)


SEARCH_FILE_MAGIC = b"PYANISX\0"
SEARCH_FILE_VERSION = 1
SEARCH_FILE_PROBE_INPUT = 0x9E3779B9          # the probe word of the header is mix32 of this: another hash refuses the file
SEARCH_FILE_ALIGN = 64
# the header: magic 8s | version, kmer, scale, n, N_BINS, n_slices uint32 | probe uint32, reserved uint32 | D, E, keys, labels' bytes uint64
_SEARCH_HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("kmer", "<u4"), ("scale", "<u4"), ("n", "<u4"), ("n_bins", "<u4"), ("n_slices", "<u4"),
                           ("probe", "<u4"), ("reserved", "<u4"), ("D", "<u8"), ("E", "<u8"), ("keys", "<u8"), ("label_bytes", "<u8")])


def search_file_probe() -> int:
    return int(mix32(np.array([SEARCH_FILE_PROBE_INPUT], dtype=np.uint32))[0])


def _search_file_layout(n, d, e, s, label_bytes):
    """[(name, dtype, count, offset)] of the file's arrays, each at the next multiple of 64 bytes behind the one before, and the file's size."""
    at = _SEARCH_HEADER.itemsize
    out = []
    for name, dtype, count in (("sizes", "<u4", n), ("lengths", "<u8", n), ("kmer", "<u4", d), ("start", "<u8", d + 1), ("member", "<u4", e),
                               ("slice_first", "<u8", s + 1), ("bin_slice", "<u4", N_BINS), ("labels", "u1", label_bytes)):
        at = -(-at // SEARCH_FILE_ALIGN) * SEARCH_FILE_ALIGN
        out.append((name, np.dtype(dtype), int(count), at))
        at += int(count) * np.dtype(dtype).itemsize
    return out, at


def write_search_index(path, shape, arrays, sizes, labels, lengths) -> int:
    """One little-endian file of a search index (DESIGN.md §16.7 has the layout): shape = (n, kmer, scale, D, E, n_slices, keys), arrays =
    (kmer, start, member, slice_first, bin_slice) as Engine.screen_search_index_export gives them, sizes uint32[n], the n labels (a label
    with a newline is a ValueError), lengths uint64[n] (the genomes' lengths; None: zeros).  Written to path + ".tmp" and renamed on
    success: a failure part-way leaves no file at `path` and none at path + ".tmp".  Returns the file's bytes."""
    import os
    n, k, scale, d, e, s, keys = (int(x) for x in shape)
    labels = [str(x) for x in labels]
    if any("\n" in x for x in labels):
        raise ValueError("a label with a newline cannot be stored in a search index file")
    lengths = np.zeros(n, dtype=np.uint64) if lengths is None else np.asarray(lengths, dtype=np.uint64).reshape(-1)
    blob = "\n".join(labels).encode("utf-8")
    given = dict(zip(("kmer", "start", "member", "slice_first", "bin_slice"), arrays), sizes=sizes, lengths=lengths, labels=np.frombuffer(blob, dtype=np.uint8))
    layout, total = _search_file_layout(n, d, e, s, len(blob))
    if len(labels) != n:
        raise ValueError(f"{len(labels)} labels for a search index of {n} genomes")
    for name, dtype, count, _ in layout:
        if len(given[name]) != count:
            raise ValueError(f"the array {name} has {len(given[name])} elements where the shape gives {count}")
    head = np.zeros(1, dtype=_SEARCH_HEADER)
    head["magic"], head["version"], head["kmer"], head["scale"], head["n"], head["n_bins"], head["n_slices"] = SEARCH_FILE_MAGIC, SEARCH_FILE_VERSION, k, scale, n, N_BINS, s
    head["probe"], head["D"], head["E"], head["keys"], head["label_bytes"] = search_file_probe(), d, e, keys, len(blob)
    tmp = str(path) + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(head.tobytes())
            for name, dtype, count, at in layout:
                f.write(b"\0" * (at - f.tell()))
                np.ascontiguousarray(given[name], dtype=dtype).tofile(f)
            if f.tell() != total:
                raise OSError(f"wrote {f.tell()} bytes of a search index file of {total}")
        os.replace(tmp, str(path))
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return total


class SearchIndexFile(NamedTuple):
    """What read_search_index gives: the arrays are read-only np.memmap views of the file (a 12 GB index is not held twice on the host)."""
    shape: Tuple[int, int, int, int, int, int, int]      # n, kmer, scale, D, E, n_slices, keys
    arrays: Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]      # kmer, start, member, slice_first, bin_slice
    sizes: np.ndarray           # uint32[n], as STORED: the import computes them again and the two are compared
    labels: List[str]
    lengths: np.ndarray         # uint64[n]


def read_search_index(path) -> SearchIndexFile:
    """The file write_search_index wrote, through np.memmap.  ValueError, naming what is wrong: a wrong magic, version, N_BINS or probe
    word, a file shorter or longer than its header implies, a label count other than n.  The CONTENT of the arrays is not judged here:
    the import validates it on the device (check_search_index states how)."""
    import os
    path = str(path)
    size = os.path.getsize(path)
    if size < _SEARCH_HEADER.itemsize:
        raise ValueError(f"{path}: {size} bytes are too few for the header of a search index file")
    head = np.fromfile(path, dtype=_SEARCH_HEADER, count=1)[0]
    if bytes(head["magic"]).ljust(8, b"\0") != SEARCH_FILE_MAGIC:
        raise ValueError(f"{path}: not a search index file (wrong magic)")
    if int(head["version"]) != SEARCH_FILE_VERSION:
        raise ValueError(f"{path}: search index file of version {int(head['version'])}, not {SEARCH_FILE_VERSION}")
    if int(head["n_bins"]) != N_BINS:
        raise ValueError(f"{path}: search index file with {int(head['n_bins'])} slice bins (N_BINS), not {N_BINS}")
    if int(head["probe"]) != search_file_probe():
        raise ValueError(f"{path}: the probe word of the file is not this build's hash of its constant: the file's k-mers were sampled by another hash")
    n, k, scale, s = (int(head[x]) for x in ("n", "kmer", "scale", "n_slices"))
    d, e, keys, label_bytes = (int(head[x]) for x in ("D", "E", "keys", "label_bytes"))
    layout, total = _search_file_layout(n, d, e, s, label_bytes)
    if size != total:
        raise ValueError(f"{path}: {size} bytes where the header implies {total}: the file is {'shorter' if size < total else 'longer'} than its header says")
    got = {name: (np.memmap(path, dtype=dtype, mode="r", offset=at, shape=(count,)) if count else np.zeros(0, dtype=dtype)) for name, dtype, count, at in layout}
    blob = bytes(got["labels"])
    labels = blob.decode("utf-8").split("\n") if n else []
    if len(labels) != n or (n == 0 and blob):
        raise ValueError(f"{path}: {len(labels) if n else 1} labels for {n} genomes")
    return SearchIndexFile((n, k, scale, d, e, s, keys), (got["kmer"], got["start"], got["member"], got["slice_first"], got["bin_slice"]), got["sizes"], labels,
                           got["lengths"])


class SearchHits(NamedTuple):
    """The cells a search kept (Engine.screen_search), row-major: a = the position in `query_labels`, b = the position in `db_labels`,
    shared = |S(query a) & S(db b)|.  An ESTIMATE, as every frame of the screen."""
    query_labels: List[str]
    db_labels: List[str]
    options: ScreenOptions
    query_sizes: np.ndarray     # uint32[q]
    db_sizes: np.ndarray        # uint32[n]
    a: np.ndarray               # int32[m]
    b: np.ndarray               # int32[m]
    shared: np.ndarray          # uint32[m]

    def pairs(self) -> List[Tuple[int, int]]:
        return list(zip(self.a.tolist(), self.b.tolist()))

    def _containment(self, size) -> np.ndarray:
        size = size.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(size > 0, self.shared.astype(np.float64) / size, np.nan)

    def containment_query(self) -> np.ndarray:
        """shared / |S(query)|: the share of the query's sampled k-mers found in the db genome (NaN for an empty query)."""
        return self._containment(self.query_sizes[self.a])

    def containment_db(self) -> np.ndarray:
        """shared / |S(db genome)| (NaN for an empty db genome)."""
        return self._containment(self.db_sizes[self.b])

    def identity(self) -> np.ndarray:
        """The quantity the rule thresholds: the LARGER of the two containments to the power 1 / k where shared >= min_shared, else 0.0
        (each side by _identity_of_counts, the very expression identity_thresholds bisects)."""
        out = np.zeros(len(self.shared), dtype=np.float64)
        for size in (self.query_sizes[self.a], self.db_sizes[self.b]):
            ok = (self.shared >= self.options.min_shared) & (size > 0)
            side = np.zeros(len(out), dtype=np.float64)
            side[ok] = _identity_of_counts(self.shared[ok], size[ok], self.options.kmer)
            out = np.maximum(out, side)
        return out

    def frame(self) -> pd.DataFrame:
        """One row per kept cell: query, db (labels), shared, containment_query, containment_db, identity."""
        ql, dl = np.array(list(self.query_labels), dtype=object), np.array(list(self.db_labels), dtype=object)
        return pd.DataFrame({"query": ql[self.a] if len(self.a) else [], "db": dl[self.b] if len(self.b) else [], "shared": self.shared,
                             "containment_query": self.containment_query(), "containment_db": self.containment_db(), "identity": self.identity()})

    def best(self, top: int = 1) -> "SearchHits":
        """Per query its `top` hits by identity, the best first, ties to the smaller db index (host numpy); a query without a hit has none."""
        if isinstance(top, bool) or int(top) != top or int(top) < 1:
            raise ValueError(f"top must be an integer >= 1, not {top!r}")
        order = np.lexsort((self.b, -self.identity(), self.a))      # by query, then identity descending, then db index ascending
        a = self.a[order]
        first = np.searchsorted(a, a, side="left")                  # the first position of every entry's query
        keep = order[np.arange(len(a)) - first < int(top)]
        return self._replace(a=self.a[keep], b=self.b[keep], shared=self.shared[keep])


def search_chunks(engine, query_ids, options) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(query sizes, a, b, shared) of the queries against the engine's resident search index: chunks of band_rows queries, each counted
    (Engine.screen_search_count), given its thresholds and selected; the chunk's row offset is added.  options.kmer and options.scale
    must be the index's.  The index stays resident."""
    options = check_options(options)
    info = getattr(engine, "_search", None)
    if not info or not info["n"]:
        raise ValueError("no search index on this engine (call screen_search_index first)")
    if (options.kmer, options.scale) != (info["kmer"], info["scale"]):
        raise ValueError(f"the search index was built with kmer {info['kmer']} and scale {info['scale']}, not {options.kmer} and {options.scale}")
    query_ids = [int(i) for i in query_ids]
    rows = int(getattr(engine, "_band_rows", 0)) or default_search_rows(info["n"])
    need_db = identity_thresholds(info["sizes"], options.kmer, options.min_identity, options.min_shared)
    sizes, parts = [np.zeros(0, np.uint32)], [(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))]
    for c0 in range(0, len(query_ids), rows):
        size = engine.screen_search_count(query_ids[c0:c0 + rows])
        need_q = identity_thresholds(size, options.kmer, options.min_identity, options.min_shared)
        a, b, s = engine.screen_search_select(need_q, need_db)
        sizes.append(size)
        parts.append((a + np.int32(c0), b, s))
    return (np.concatenate(sizes), *(np.concatenate([p[i] for p in parts]) for i in range(3)))


def search_labels(ids, labels, what: str) -> List[str]:
    labels = [str(x) for x in (ids if labels is None else labels)]
    if len(labels) != len(ids):
        raise ValueError(f"{what} ids and labels must have the same length")
    return labels


# ---- the gather: a query decomposed into the collection's genomes ----------------------------------------------------------
GATHER_MAX_RANKS = 65536


class GatherOptions(NamedTuple):
    """What a gather asks: a db genome is worth a row while it explains at least max(min_unique, ceil(min_fraction * |S(query)|)) of the
    query's sampled k-mers that no better match has explained; at most max_ranks rows per query.  There is no default min_unique: two
    unrelated 5 Mb genomes share about 50 sampled 16-mers by chance at scale 256, so the right floor depends on the genomes' size and
    the scale.  abundance: the count also keeps how many times the query holds each matched k-mer, and every row gets
    the statistics of the multiplicities of the k-mers it claimed; the rows themselves do not change."""
    kmer: int
    scale: int
    min_unique: int
    min_fraction: float = 0.0
    max_ranks: int = GATHER_MAX_RANKS
    abundance: bool = False


def check_gather_options(options) -> GatherOptions:
    """A GatherOptions validated (no library call): kmer and scale as check_params, min_unique an integer >= 1, min_fraction a real number
    in [0, 1], max_ranks an integer 1 ... 65536, abundance a bool."""
    if not isinstance(options, GatherOptions):
        raise ValueError(f"gather options are a GatherOptions, not {options!r}")
    kmer, scale = check_params(options.kmer, options.scale)
    mu, mf, mr = options.min_unique, options.min_fraction, options.max_ranks
    if isinstance(mu, bool) or not isinstance(mu, (int, np.integer)) or not 1 <= int(mu) < (1 << 32):
        raise ValueError(f"min_unique must be an integer >= 1 (below 2^32), not {mu!r}")
    if isinstance(mf, bool) or not isinstance(mf, (int, float, np.integer, np.floating)) or math.isnan(float(mf)) or not 0.0 <= float(mf) <= 1.0:
        raise ValueError(f"min_fraction must be a number in [0, 1], not {mf!r}")
    if isinstance(mr, bool) or not isinstance(mr, (int, np.integer)) or not 1 <= int(mr) <= GATHER_MAX_RANKS:
        raise ValueError(f"max_ranks must be an integer 1 ... {GATHER_MAX_RANKS}, not {mr!r}")
    if not isinstance(options.abundance, (bool, np.bool_)):
        raise ValueError(f"abundance must be True or False, not {options.abundance!r}")
    return GatherOptions(kmer, scale, int(mu), float(mf), int(mr), bool(options.abundance))


def gather_thresholds(query_sizes, min_unique: int, min_fraction: float = 0.0) -> np.ndarray:
    """need uint32[q] = max(min_unique, ceil(min_fraction * size)), floored at 1: the smallest unique count worth a row.  The product is
    taken in float64 (sizes are below 2^32: exact operands) and rounded up."""
    sizes = np.ascontiguousarray(query_sizes, dtype=np.uint32).reshape(-1)
    if isinstance(min_unique, bool) or int(min_unique) != min_unique or not 0 <= int(min_unique) < (1 << 32):
        raise ValueError(f"min_unique must be an integer 0 ... 2^32 - 1, not {min_unique!r}")
    if isinstance(min_fraction, bool) or math.isnan(float(min_fraction)) or not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError(f"min_fraction must be a number in [0, 1], not {min_fraction!r}")
    part = np.ceil(float(min_fraction) * sizes.astype(np.float64)).astype(np.uint64)
    return np.maximum(np.maximum(part, np.uint64(int(min_unique))), np.uint64(1)).astype(np.uint32)


class GatherResult(NamedTuple):
    """The rows of a gather (Engine.screen_gather), ordered by query, then rank: query = the position in `query_labels`, db = the position
    in `db_labels`, unique = the query's k-mers this genome explains that no row before it explained, total = |S(query) & S(db)|.  An
    ESTIMATE, as every frame of the screen."""
    query_labels: List[str]
    db_labels: List[str]
    options: GatherOptions
    query_sizes: np.ndarray     # uint32[q]
    db_sizes: np.ndarray        # uint32[n]
    query: np.ndarray           # int32[r]
    db: np.ndarray              # int32[r]
    unique: np.ndarray          # uint32[r]
    total: np.ndarray           # uint32[r]
    matched: np.ndarray         # uint32[q]: |S(query) & the union of the db|, the entries the count kept
    # options.abundance only (None otherwise): a(i, x) = the times query i holds the sampled k-mer x
    query_weight: Optional[np.ndarray] = None       # uint64[q]: W, the sum of a over S(query)
    matched_weight: Optional[np.ndarray] = None     # uint64[q]: MW, the sum of a over the matched entries
    sum_abund: Optional[np.ndarray] = None          # uint64[r]: over the k-mers the row claimed (`unique` of them): the sum of a,
    sumsq_abund: Optional[np.ndarray] = None        # object[r]: the sum of a^2 as Python ints (sumsq_words joins the library's two words),
    median2_abund: Optional[np.ndarray] = None      # uint64[r]: twice the median,
    min_abund: Optional[np.ndarray] = None          # uint32[r]
    max_abund: Optional[np.ndarray] = None          # uint32[r]

    def has_abundance(self) -> bool:
        return self.sum_abund is not None

    def ranks(self) -> np.ndarray:
        """The rank of every row inside its query, 0 first (the rows of a query stand together)."""
        q = np.asarray(self.query)
        return (np.arange(len(q)) - np.searchsorted(q, q, side="left")).astype(np.int64)

    def frame(self) -> pd.DataFrame:
        """One row per recorded genome: query, rank, db (labels), unique, total, f_unique_query = unique / |S(query)|, f_unique_cumulative
        = its running sum inside the query, f_match = total / |S(db)|, identity = f_match ** (1 / k)."""
        ql, dl = np.array(list(self.query_labels), dtype=object), np.array(list(self.db_labels), dtype=object)
        qsize, dsize = self.query_sizes[self.query].astype(np.float64), self.db_sizes[self.db].astype(np.float64)
        unique = self.unique.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f_unique = np.where(qsize > 0, unique / qsize, np.nan)
            f_match = np.where(dsize > 0, self.total.astype(np.float64) / dsize, np.nan)
        running = np.cumsum(self.unique.astype(np.int64))
        first = np.searchsorted(self.query, self.query, side="left")
        before = np.where(first > 0, running[np.maximum(first, 1) - 1], 0) if len(running) else running
        with np.errstate(divide="ignore", invalid="ignore"):
            f_running = np.where(qsize > 0, (running - before).astype(np.float64) / qsize, np.nan)
        frame = pd.DataFrame({"query": ql[self.query] if len(self.query) else [], "rank": self.ranks(), "db": dl[self.db] if len(self.db) else [],
                              "unique": self.unique, "total": self.total, "f_unique_query": f_unique, "f_unique_cumulative": f_running,
                              "f_match": f_match, "identity": np.power(f_match, 1.0 / self.options.kmer)})
        if self.has_abundance():      # with the abundances: average_abund, median_abund, std_abund, f_unique_weighted, f_weighted_cumulative
            for name, column in abundance_columns(self.query, self.unique, self.sum_abund, self.sumsq_abund, self.median2_abund, self.query_weight).items():
                frame[name] = column
        return frame

    def summary(self) -> pd.DataFrame:
        """One row per query: query, size, matched = |S(query) & the union of the db|, rows, explained = the sum of its rows' unique,
        unexplained = matched - explained: the k-mers that matched the collection but stayed below the threshold (or beyond max_ranks)."""
        q = len(self.query_labels)
        rows = np.bincount(self.query, minlength=q).astype(np.int64)
        explained = np.bincount(self.query, weights=self.unique.astype(np.float64), minlength=q).astype(np.int64)      # (sums below 2^53: exact)
        matched = self.matched.astype(np.int64)
        frame = pd.DataFrame({"query": list(self.query_labels), "size": self.query_sizes.astype(np.int64), "matched": matched, "rows": rows,
                              "explained": explained, "unexplained": matched - explained})
        if self.has_abundance():      # weight = W, matched_weight = MW, explained_weight = the rows' sum_abund, unexplained_weight = MW - that
            told = [0] * q
            for i, x in zip(self.query.tolist(), self.sum_abund.tolist()):
                told[i] += int(x)
            frame["weight"] = np.asarray(self.query_weight, dtype=np.uint64)
            frame["matched_weight"] = np.asarray(self.matched_weight, dtype=np.uint64)
            frame["explained_weight"] = np.array(told, dtype=np.uint64)
            frame["unexplained_weight"] = np.array([int(m) - t for m, t in zip(self.matched_weight.tolist(), told)], dtype=np.uint64)
        return frame


def sumsq_words(words) -> np.ndarray:
    """The sums of squares of pg_screen_gather_abund_read, uint64[r, 2] = (lo, hi) words, as an object array of Python ints."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1, 2)
    out = np.empty(len(words), dtype=object)
    for j, (lo, hi) in enumerate(words.tolist()):
        out[j] = int(lo) + (int(hi) << 64)
    return out


def abundance_columns(query, unique, sum_abund, sumsq_abund, median2_abund, query_weight) -> dict:
    """The float columns of a gather's abundances from its integers, with Python integers throughout (true division of two ints is
    correctly rounded, so every column is a fixed function of the integers): average_abund = sum / m, median_abund = median2 / 2,
    std_abund = sqrt((m sumsq - sum^2) / m^2) (the population form, as numpy.std), f_unique_weighted = sum / W[query],
    f_weighted_cumulative = (the sum of `sum` over the query's rows so far) / W[query].  m = unique; NaN where a divisor is 0."""
    nan = float("nan")
    average, median, std, f_weighted, f_running = [], [], [], [], []
    running, before = 0, None
    weight = [int(w) for w in np.asarray(query_weight).tolist()]
    for i, m, total, sq, med2 in zip(np.asarray(query).tolist(), np.asarray(unique).tolist(), np.asarray(sum_abund).tolist(), list(sumsq_abund),
                                     np.asarray(median2_abund).tolist()):
        m, total, sq, med2 = int(m), int(total), int(sq), int(med2)
        running = total if i != before else running + total
        before = i
        average.append(total / m if m else nan)
        median.append(med2 / 2)
        std.append(math.sqrt((m * sq - total * total) / (m * m)) if m and m * sq >= total * total else nan)
        f_weighted.append(total / weight[i] if weight[i] else nan)
        f_running.append(running / weight[i] if weight[i] else nan)
    return {"average_abund": np.array(average, dtype=np.float64), "median_abund": np.array(median, dtype=np.float64),
            "std_abund": np.array(std, dtype=np.float64), "f_unique_weighted": np.array(f_weighted, dtype=np.float64),
            "f_weighted_cumulative": np.array(f_running, dtype=np.float64)}


def gather_chunks(engine, query_ids, options):
    """(query sizes, matched, query, db, unique, total) of the queries against the engine's resident search index: chunks of band_rows
    queries, each counted with its entries kept (Engine.screen_gather_count), given its thresholds and decomposed; the chunk's row
    offset is added.  options.kmer and options.scale must be the index's.  The index stays resident; the last chunk's rectangle, entries
    and rows are dropped before this returns, on errors too (a count of no queries).  With options.abundance seven more follow, in the
    order of GatherResult's trailing fields: every chunk is counted with its abundances kept and the abundance pass runs after its
    rounds (the pass's rank table is a third array of the rectangle's size beside the rectangle and its working copy)."""
    options = check_gather_options(options)
    info = getattr(engine, "_search", None)
    if not info or not info["n"]:
        raise ValueError("no search index on this engine (call screen_search_index first)")
    if (options.kmer, options.scale) != (info["kmer"], info["scale"]):
        raise ValueError(f"the search index was built with kmer {info['kmer']} and scale {info['scale']}, not {options.kmer} and {options.scale}")
    query_ids = [int(i) for i in query_ids]
    rows = int(getattr(engine, "_band_rows", 0)) or default_search_rows(info["n"])
    sizes, matched = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    parts = [(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))]
    weights = [(np.zeros(0, np.uint64), np.zeros(0, np.uint64))]
    stats = [(np.zeros(0, np.uint64), np.zeros(0, object), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))]
    try:
        for c0 in range(0, len(query_ids), rows):
            if options.abundance:
                size, weight = engine.screen_gather_count(query_ids[c0:c0 + rows], abundance=True)
                weights.append((weight, engine.screen_gather_abundance_matched()))
            else:
                size = engine.screen_gather_count(query_ids[c0:c0 + rows])
            matched.append(engine.screen_gather_matched())
            qi, db, unique, total = engine.screen_gather_rows(gather_thresholds(size, options.min_unique, options.min_fraction), options.max_ranks)
            if options.abundance:
                a_sum, a_sumsq, a_median2, a_min, a_max = engine.screen_gather_abundance()
                stats.append((a_sum, sumsq_words(a_sumsq), a_median2, a_min, a_max))
            sizes.append(size)
            parts.append((qi + np.int32(c0), db, unique, total))
    finally:
        try:
            engine.screen_search_count([])
        except Exception:      # (the first error is the one to report)
            pass
    plain = (np.concatenate(sizes), np.concatenate(matched), *(np.concatenate([p[i] for p in parts]) for i in range(4)))
    if not options.abundance:
        return plain
    return (*plain, *(np.concatenate([w[i] for w in weights]) for i in range(2)), *(np.concatenate([t[i] for t in stats]) for i in range(5)))
