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

An ESTIMATE for triage with its own frames: it is never written into an exact ANIm / ANIb matrix.  What this is modelled on: the
sketch-then-align front ends of skani, sourmash and dRep; pyani itself has no such step.
"""
import math
from typing import List, NamedTuple, Sequence, Tuple

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
