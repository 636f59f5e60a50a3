"""The gather's statement in plain Python sets and numpy, and the inputs of its tests (tests/test_screen_gather_cpu.py,
tests/test_screen_gather_gpu.py).  For a query Q and db sets S(0) ... S(n - 1): R = Q; per round left[b] = |R & S(b)|, the winner is the
SMALLEST b with the largest left[b]; the query stops when left[w] < need or it has max_ranks rows; otherwise the row (rank, w, unique =
left[w], total = |Q & S(w)|) is recorded and R loses S(w).  The k-mer sets come from tests/screen_cases.genome_set, unchanged.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file, and nothing here imports pyani_amd."""
import functools
from typing import NamedTuple

import numpy as np

from tests import screen_cases as scr
from tests import sketch_cases as sc


class Gathered(NamedTuple):
    query: np.ndarray        # int32[r]   the rows, by query, then rank
    db: np.ndarray           # int32[r]
    unique: np.ndarray       # uint32[r]
    total: np.ndarray        # uint32[r]
    hits: np.ndarray         # uint32[q, n]   the rectangle
    left: np.ndarray         # uint32[q, n]   what the rounds left of it
    matched: np.ndarray      # uint32[q]      |Q & the union of the db|
    claimed: int             # k-mers that left a query with a winner
    decrements: int          # the db holders of those k-mers, summed
    rounds: int              # the last round in which a query was unfinished: max rows + 1 (0 without a query)


def gather_sets(query_sets, db_sets, need, max_ranks):
    """The statement over Python sets: query_sets, db_sets = lists of iterables of k-mers; need = one int >= 1 per query."""
    db = [set(int(x) for x in s) for s in db_sets]
    n, q = len(db), len(query_sets)
    holders = {}
    for b, s in enumerate(db):
        for x in s:
            holders.setdefault(x, []).append(b)
    rows, hits, left = [], np.zeros((q, n), dtype=np.uint32), np.zeros((q, n), dtype=np.uint32)
    matched = np.zeros(q, dtype=np.uint32)
    claimed = decrements = rounds = 0
    for i, qs in enumerate(query_sets):
        full = set(int(x) for x in qs)
        rest = {x for x in full if x in holders}
        matched[i] = len(rest)
        hits[i] = [len(full & s) for s in db]
        rank = 0
        while True:
            now = [len(rest & s) for s in db]
            w = max(range(n), key=lambda b: (now[b], -b))
            if now[w] < max(1, int(need[i])) or rank >= max_ranks:
                break
            rows.append((i, w, now[w], int(hits[i, w])))
            gone = rest & db[w]
            claimed += len(gone)
            decrements += sum(len(holders[x]) for x in gone)
            rest -= gone
            rank += 1
        rounds = max(rounds, rank + 1)
        left[i] = [len(rest & s) for s in db]
    cols = list(zip(*rows)) if rows else [(), (), (), ()]
    return Gathered(np.array(cols[0], dtype=np.int32), np.array(cols[1], dtype=np.int32), np.array(cols[2], dtype=np.uint32),
                    np.array(cols[3], dtype=np.uint32), hits, left, matched, claimed, decrements, rounds)


def gather_genomes(queries, db, k, scale, need, max_ranks=65536):
    """The statement for genomes [(seq, rec_off)]: need = an int for every query, or one per query."""
    qsets = [scr.genome_set(s, o, k, scale) for s, o in queries]
    need = [need] * len(queries) if np.isscalar(need) else list(need)
    return gather_sets(qsets, [scr.genome_set(s, o, k, scale) for s, o in db], need, max_ranks)


def check_consequences(g: Gathered, n, max_ranks):
    """What the definition implies, for any Gathered (the statement's or the device's rows put into one)."""
    for i in range(len(g.hits)):
        mine = g.query == i
        u, t, w = g.unique[mine].astype(np.int64), g.total[mine].astype(np.int64), g.db[mine]
        assert (np.diff(u) <= 0).all() and (u <= t).all() and (u >= 1).all(), (i, u, t)
        assert len(w) <= min(n, max_ranks) and len(set(w.tolist())) == len(w), (i, w)
        assert (g.left[i, w] == 0).all(), (i, w, g.left[i, w])
        assert (g.left[i] <= g.hits[i]).all()
        assert int(u.sum()) <= int(g.matched[i])
    assert (np.diff(g.query) >= 0).all()


def join(genomes):
    """One multi-record genome of all the records of several: (seq, rec_off)."""
    seqs, off, base = [], [0], 0
    for s, o in genomes:
        seqs.append(np.asarray(s, dtype=np.uint8))
        off += [base + int(x) for x in o[1:]]
        base += int(o[-1])
    return np.concatenate(seqs), np.array(off, dtype=np.uint64)


def same_rows(got, want: Gathered, what):
    for g, w, dtype, name in zip(got, (want.query, want.db, want.unique, want.total), (np.int32, np.int32, np.uint32, np.uint32), ("query", "db", "unique", "total")):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape, g[:8], w[:8])
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


# ---- mixture: the family's genomes 3 and 7 and 60 kb of new sequence in one genome; genomes 1 and 5 as further queries ----------------------
MIXTURE_MEMBERS, MIXTURE_FRESH = (3, 7), 60_000


@functools.lru_cache(maxsize=None)
def mixture_queries():
    fam = scr.family()
    rng = np.random.default_rng(20261905)
    fresh = (sc.random_bases(rng, MIXTURE_FRESH), np.array([0, MIXTURE_FRESH], dtype=np.uint64))
    return [join([fam[3], fam[7], fresh]), fam[1], fam[5]]


@functools.lru_cache(maxsize=None)
def mixture_expected(k, scale, need=1, max_ranks=65536):
    return gather_genomes(mixture_queries(), scr.family(), k, scale, need, max_ranks)


# ---- wide: the records of genomes 0 and 4 of the 3000 in one query ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_query():
    g = scr.wide()
    return join([g[0], g[4]])


@functools.lru_cache(maxsize=None)
def wide_expected():
    k, scale = scr.WIDE_PARAMS
    return gather_genomes([wide_query()], scr.wide(), k, scale, 1)


# ---- many ranks: 40 unrelated genomes of 2000 + 50 j bases, one query that holds them all ---------------------------------------------------
MANY_N, MANY_PARAMS = 40, (16, 1)


@functools.lru_cache(maxsize=None)
def many():
    rng = np.random.default_rng(20261906)
    return [(sc.random_bases(rng, 2000 + 50 * j), np.array([0, 2000 + 50 * j], dtype=np.uint64)) for j in range(MANY_N)]


@functools.lru_cache(maxsize=None)
def many_expected(need=1, max_ranks=65536):
    k, scale = MANY_PARAMS
    return gather_genomes([join(many())], many(), k, scale, need, max_ranks)
