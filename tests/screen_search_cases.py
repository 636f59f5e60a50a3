"""The search's expected values (tests/test_screen_search_cpu.py, tests/test_screen_search_gpu.py and the multi-engine and driver tests):
blocks of the screen's numpy statement (tests/screen_cases.py) and the selection rule on a block as one numpy expression.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file, and nothing here imports pyani_amd."""
import numpy as np

from tests import screen_cases as scr

FAMILY_DB, FAMILY_QUERIES = [0, 3, 4, 5, 7], [1, 2, 6, 7]      # genome 7 is on both sides: it meets itself, a cell like any other
EDGES_DB, EDGES_QUERIES = [0, 1, 5], [2, 3, 4, 1]              # queries: shorter than k, N only, the twin of db genome 0, a db member
# the kept cells at screen_select_cases.THRESHOLDS with min_shared = 2, worked out from the statement on the CPU (the CPU test asserts them)
FAMILY_KEPT = {(16, 16): (20, 13, 13, 12, 3, 3), (12, 16): (20, 20, 13, 12, 3, 3)}
EDGES_KEPT = (12, 4, 4, 4, 2, 2)


def block(case, k, scale, queries, db):
    """(query sizes, db sizes, hits uint32[q, n]) of the statement over the case's genomes: the block shared[queries x db]."""
    sizes, shared = scr.expected(case, k, scale)
    return sizes[queries], sizes[db], np.ascontiguousarray(shared[np.ix_(queries, db)])


def rule_block(hits, need_q, need_db):
    """(a, b, hits[a][b]) of the cells with hits[a][b] >= min(need_q[a], need_db[b]), row-major: the rule of screen_select_cases.rule on a
    rectangle, where no cell is a diagonal."""
    hits = np.asarray(hits, dtype=np.uint32)
    keep = hits >= np.minimum.outer(np.asarray(need_q, dtype=np.uint32), np.asarray(need_db, dtype=np.uint32))
    a, b = np.nonzero(keep)
    return a.astype(np.int32), b.astype(np.int32), hits[a, b]


def restricted(shared, need, queries, db):
    """The cells (a in queries, b in db) that the all-vs-all rule keeps over ALL genomes, re-indexed to positions in `queries` and `db`,
    row-major; a genome on both sides keeps the cell with itself iff its size reaches its own threshold (the all-vs-all rule has no
    such cell: it is the one thing a rectangle adds)."""
    shared = np.asarray(shared, dtype=np.uint32)
    need = np.asarray(need, dtype=np.uint32)
    keep = shared >= np.minimum.outer(need, need)
    sub = keep[np.ix_(queries, db)]
    a, b = np.nonzero(sub)
    return a.astype(np.int32), b.astype(np.int32), shared[np.asarray(queries)[a], np.asarray(db)[b]]


def same(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.int32, np.uint32), "abs"):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
