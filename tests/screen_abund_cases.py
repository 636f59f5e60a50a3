"""The statement of the gather's abundances in Python integers, and the inputs of its tests
(tests/test_screen_gather_abund_cpu.py, tests/test_screen_gather_abund_gpu.py).  a(i, x) = the times query i holds the sampled
canonical k-mer x: tests/screen_cases.genome_occurrences counted by numpy.unique.  The rows are those of the unweighted statement,
tests/screen_gather_cases.gather_sets, unchanged: abundance does not move a winner.  The claimed set of row (i, t) is re-derived from the
rows, C(i, t) = (Q & S(w_t)) minus the sets of the winners before it, and must hold `unique` k-mers; the statistics are over a(i, x), x in
C(i, t), with Python ints and the sorted list.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file, and nothing here imports pyani_amd."""
import functools
import math
from typing import List, NamedTuple

import numpy as np

from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import sketch_cases as sc


class Abundances(NamedTuple):
    gathered: sgc.Gathered       # the rows, the rectangle and the counters of the unweighted statement
    weight: List[int]            # W[i]: the sum of a(i, x) over S(query i)
    matched_weight: List[int]    # MW[i]: the same over the matched k-mers
    sum: List[int]               # per row, in the rows' order
    sumsq: List[int]
    median2: List[int]
    min: List[int]
    max: List[int]
    unattributed: int            # matched (query, k-mer) entries that belong to no row
    holders: int                 # the db holders of every matched entry, summed: what the attribution walks


def counts_of(seq, rec_off, k, scale):
    """{k-mer: a} of one genome."""
    kmers, counts = np.unique(scr.genome_occurrences(seq, rec_off, k, scale), return_counts=True)
    return {int(x): int(c) for x, c in zip(kmers.tolist(), counts.tolist())}


def abundance_sets(query_counts, db_sets, need, max_ranks, gathered=None) -> Abundances:
    """The statement over dicts {k-mer: multiplicity} (the queries) and iterables of k-mers (the db); need = one int >= 1 per query.
    gathered: the rows of gather_sets over the same sets, where a test already has them."""
    db = [set(int(x) for x in s) for s in db_sets]
    g = gathered if gathered is not None else sgc.gather_sets([list(c) for c in query_counts], db, need, max_ranks)
    holders = {}
    for s in db:
        for x in s:
            holders[x] = holders.get(x, 0) + 1
    weight = [sum(c.values()) for c in query_counts]
    matched_weight = [sum(a for x, a in c.items() if x in holders) for c in query_counts]
    walked = sum(holders[x] for c in query_counts for x in c if x in holders)
    out = ([], [], [], [], [])
    attributed = 0
    for i, counts in enumerate(query_counts):
        taken = set()
        for w, unique in zip(g.db[g.query == i].tolist(), g.unique[g.query == i].tolist()):
            claimed = (set(counts) & db[w]) - taken
            assert len(claimed) == unique, (i, w, len(claimed), unique)
            taken |= db[w]
            a = sorted(counts[x] for x in claimed)
            m = len(a)
            attributed += m
            for column, value in zip(out, (sum(a), sum(x * x for x in a), a[(m - 1) // 2] + a[m // 2], a[0], a[-1])):
                column.append(value)
    matched = sum(1 for c in query_counts for x in c if x in holders)
    assert matched == int(g.matched.astype(np.int64).sum())
    return Abundances(g, weight, matched_weight, *out, matched - attributed, walked)


def abundance_genomes(queries, db, k, scale, need, max_ranks=65536, gathered=None) -> Abundances:
    """The statement for genomes [(seq, rec_off)]: need = an int for every query, or one per query."""
    need = [need] * len(queries) if np.isscalar(need) else list(need)
    return abundance_sets([counts_of(s, o, k, scale) for s, o in queries], [scr.genome_set(s, o, k, scale) for s, o in db], need, max_ranks, gathered)


def columns(want: Abundances):
    """The host columns from the statement's integers: {name: [float per row]} (Python ints: true division is correctly rounded)."""
    g = want.gathered
    out = {"average_abund": [], "median_abund": [], "std_abund": [], "f_unique_weighted": [], "f_weighted_cumulative": []}
    running = {}
    for i, m, s, sq, med2 in zip(g.query.tolist(), g.unique.tolist(), want.sum, want.sumsq, want.median2):
        running[i] = running.get(i, 0) + s
        out["average_abund"].append(s / m)
        out["median_abund"].append(med2 / 2)
        out["std_abund"].append(math.sqrt((m * sq - s * s) / (m * m)))
        out["f_unique_weighted"].append(s / want.weight[i])
        out["f_weighted_cumulative"].append(running[i] / want.weight[i])
    return out


def summary_columns(want: Abundances):
    g = want.gathered
    explained = [0] * len(want.weight)
    for i, s in zip(g.query.tolist(), want.sum):
        explained[i] += s
    return {"weight": want.weight, "matched_weight": want.matched_weight, "explained_weight": explained,
            "unexplained_weight": [m - e for m, e in zip(want.matched_weight, explained)]}


# ---- covered: the mixture with unequal copy numbers: genome 3 three times, genome 7 once, the fresh 60 kb twice; genome 1 once and genome
# 5 twice as further queries.  The multiplicities are 3, 1, 2 and, where the members share a k-mer, 4 (and more at k 8). -----------------
@functools.lru_cache(maxsize=None)
def covered_queries():
    fam = scr.family()
    seq, _ = sgc.mixture_queries()[0]
    fresh_seq = seq[len(seq) - sgc.MIXTURE_FRESH:]
    fresh = (fresh_seq, np.array([0, sgc.MIXTURE_FRESH], dtype=np.uint64))
    return [sgc.join([fam[3], fam[3], fam[3], fam[7], fresh, fresh]), fam[1], sgc.join([fam[5], fam[5]])]


@functools.lru_cache(maxsize=None)
def covered_expected(k, scale, need=1, max_ranks=65536):
    """The rows are the un-repeated mixture's: abundance does not move a winner."""
    rows = sgc.mixture_expected(k, scale, need, max_ranks)
    want = abundance_genomes(covered_queries(), scr.family(), k, scale, need, max_ranks)
    for got, plain in zip((want.gathered.query, want.gathered.db, want.gathered.unique, want.gathered.total), (rows.query, rows.db, rows.unique, rows.total)):
        assert np.array_equal(got, plain)
    return want


# ---- with queries that have no entry: one that matches nothing, one shorter than k, among others ---------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_queries():
    rng = np.random.default_rng(20261911)
    nothing = (sc.random_bases(rng, 5_000), np.array([0, 5_000], dtype=np.uint64))
    short = (sc.random_bases(rng, 10), np.array([0, 10], dtype=np.uint64))
    covered = covered_queries()
    return [covered[0], nothing, short, covered[2]]


@functools.lru_cache(maxsize=None)
def sparse_expected(k, scale, need):
    want = abundance_genomes(sparse_queries(), scr.family(), k, scale, need)
    assert want.gathered.matched[1] == 0 and want.weight[1] > 0 and want.weight[2] == 0 and want.gathered.matched[0] > 0
    return want


# ---- tiny: db genomes of 1, 2, 3 and 4 k-mers; the query holds them 5, 2, 1 and 1 times, and a record that matches nothing -------------
TINY_PARAMS = (16, 1)
TINY_COPIES = (5, 2, 1, 1)


@functools.lru_cache(maxsize=None)
def tiny():
    """(db, query): the rows have m = 4, 3, 2, 1 — both parities of the median and the one-element row."""
    rng = np.random.default_rng(20261912)
    db = [(sc.random_bases(rng, 16 + j), np.array([0, 16 + j], dtype=np.uint64)) for j in range(4)]
    other = (sc.random_bases(rng, 40), np.array([0, 40], dtype=np.uint64))
    query = sgc.join([db[j] for j, c in enumerate(TINY_COPIES) for _ in range(c)] + [other])
    return db, query


@functools.lru_cache(maxsize=None)
def tiny_expected():
    k, scale = TINY_PARAMS
    db, query = tiny()
    want = abundance_genomes([query], db, k, scale, 1)
    assert want.gathered.unique.tolist() == [4, 3, 2, 1] and want.gathered.db.tolist() == [3, 2, 1, 0]
    assert want.median2 == [2, 2, 4, 10] and want.sum == [4, 3, 4, 5] and want.unattributed == 0
    assert want.weight[0] == want.matched_weight[0] + 25      # the 40-base record's 25 k-mers match nothing
    return want


# ---- wide: the 3000-genome case with genome 0's records twice: the attribution walks k-mers of 3000 holders ----------------------------
@functools.lru_cache(maxsize=None)
def wide_query():
    g = scr.wide()
    return sgc.join([g[0], g[0], g[4]])


@functools.lru_cache(maxsize=None)
def wide_expected():
    k, scale = scr.WIDE_PARAMS
    want = abundance_genomes([wide_query()], scr.wide(), k, scale, 1, gathered=sgc.wide_expected())
    assert want.holders >= 9 * scr.WIDE_N and want.max[0] == 3 and want.min[0] == 2      # motif 1 is in genome 0 (twice) and in genome 4
    return want


# ---- many: the 40-rank case, member j present (j mod 5) + 1 times -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_query():
    return sgc.join([g for j, g in enumerate(sgc.many()) for _ in range(j % 5 + 1)])


@functools.lru_cache(maxsize=None)
def many_expected(need=1, max_ranks=65536):
    k, scale = sgc.MANY_PARAMS
    return abundance_genomes([many_query()], sgc.many(), k, scale, need, max_ranks, gathered=sgc.many_expected(need, max_ranks))
