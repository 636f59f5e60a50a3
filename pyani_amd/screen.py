"""The screen: which of the N^2 ordered pairs of a collection are worth an exact comparison (the "k-mer sketch
pre-filter").  One engine call (Engine.screen_matrix, pg_screen_matrix) gives two INTEGER arrays for all genomes at once —
sizes[a] = |S(a)|, the distinct sampled canonical k-mers of genome a (FracMinHash: mix32(k-mer) & (scale - 1) == 0), and
shared[a][b] = |S(a) & S(b)| — and everything floating-point is computed here, on the host, from those integers:

    containment[a][b] = shared[a][b] / sizes[a]                        (NaN where sizes[a] == 0; the query on the rows)
    jaccard[a][b]     = shared[a][b] / (sizes[a] + sizes[b] - shared[a][b])
    identity[a][b]    = containment[a][b] ** (1 / k)  where shared[a][b] >= min_shared, else 0.0

(a k-mer survives iff none of its k bases changed).  The floor min_shared (default 2) matters: ONE chance k-mer between two unrelated
genomes of a few thousand sampled k-mers would read as an identity above 0.5.

An ESTIMATE for triage with its own frames: it is never written into an exact ANIm / ANIb matrix.  What this is modelled on: the
sketch-then-align front ends of skani, sourmash and dRep; pyani itself has no such step.
"""
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import pandas as pd

DEFAULT_KMER, DEFAULT_SCALE, DEFAULT_MIN_SHARED = 16, 256, 2
MAX_GENOMES = 8192


def check_params(kmer, scale) -> Tuple[int, int]:
    """(kmer, scale) as ints; ValueError outside 8 <= kmer <= 16 or for a scale that is no power of two in 1 ... 65536 (no library call)."""
    if isinstance(kmer, bool) or int(kmer) != kmer or not 8 <= int(kmer) <= 16:
        raise ValueError(f"the k-mer size must be an integer 8 ... 16, not {kmer!r}")
    if isinstance(scale, bool) or int(scale) != scale or not 1 <= int(scale) <= 65536 or int(scale) & (int(scale) - 1):
        raise ValueError(f"scale must be a power of two, 1 ... 65536, not {scale!r}")
    return int(kmer), int(scale)


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
