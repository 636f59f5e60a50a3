"""The screen's selection rule in numpy, and the inputs of its tests (tests/test_screen_select_cpu.py, tests/test_screen_select_gpu.py,
tests/test_run_screened_gpu.py).  TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.  What is stated here is the rule
of DESIGN.md §16.1 — keep (a, b) iff a != b and shared[a][b] >= min(need[a], need[b]) — as one numpy expression; the CPU test proves it
equal to ScreenResult.candidate_pairs, the GPU test holds the kernel to it."""
import functools

import numpy as np

from tests import sketch_cases as sc

KMERS = (8, 12, 16)
THRESHOLDS = (0.0, 0.5, 0.8, 0.9, 0.999, 1.0)


def rule(shared, need):
    """(a, b, shared[a][b]) of the kept cells, row-major: int32, int32, uint32."""
    shared = np.asarray(shared, dtype=np.uint32)
    need = np.asarray(need, dtype=np.uint32)
    keep = shared >= np.minimum.outer(need, need)
    np.fill_diagonal(keep, False)
    a, b = np.nonzero(keep)
    return a.astype(np.int32), b.astype(np.int32), shared[a, b]


def random_symmetric(seed, n, max_size=5000):
    """sizes uint32[n] <= max_size (a few of them 0, 1 and max_size) and a symmetric uint32 matrix with shared[a][b] <= min(sizes[a],
    sizes[b]) and the diagonal = sizes: most cells small, some near the smaller size, so that every threshold splits them."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, max_size + 1, n)
    sizes[rng.integers(0, n, max(1, n // 20))] = 0
    sizes[rng.integers(0, n, max(1, n // 20))] = 1
    sizes[rng.integers(0, n)] = max_size
    cap = np.minimum.outer(sizes, sizes)
    frac = np.where(rng.random((n, n)) < 0.3, rng.random((n, n)), rng.random((n, n)) ** 8)
    frac = np.where(rng.random((n, n)) < 0.05, 1.0, frac)
    m = np.floor(frac * (cap + 1)).astype(np.int64).clip(0, cap)
    m = np.triu(m, 1)
    m = m + m.T
    m[np.arange(n), np.arange(n)] = sizes
    return sizes.astype(np.uint32), m.astype(np.uint32)


# ---- the six genomes of the screened runs ------------------------------------------------------------------------------------------------
RUN_STEMS = ("famA1", "famA2", "famA3", "famB1", "famB2", "famB3")
RUN_BASES, RUN_RATE = 60_000, 0.025      # every member 2.5 % substitutions off its family's ancestor: ~95 % identity between two members
RUN_KEPT = [(q, s) for q in RUN_STEMS for s in RUN_STEMS if q != s and q[:4] == s[:4]]      # the 12 within-family ordered pairs


@functools.lru_cache(maxsize=None)
def run_genomes():
    """Two families of three genomes of 60 kb (two records each, odd boundary), unrelated across families."""
    rng = np.random.default_rng(20261905)
    out = []
    for _ in range(2):
        anc = sc.random_bases(rng, RUN_BASES)
        for _ in range(3):
            out.append((sc.substituted(rng, anc, RUN_RATE), sc.offsets(RUN_BASES, 2, 17)))
    return out
