"""GPU (through the C ABI): the gather's abundances (pg_screen_gather_count_abund / pg_screen_gather_abund / _read / _matched / _last;
pyani_amd/csrc/pgscr_abund.inc) against the statement in Python integers (tests/screen_abund_cases.py).  Everything is an
integer and must be EQUAL — sum, both words of sumsq, median2, min, max, W and MW — and the float columns are the same expressions over
the statement's integers: no tolerance anywhere.  The abundance count must leave behind exactly what the plain gather count leaves."""
import ctypes

import numpy as np
import pytest

from tests import screen_abund_cases as sac
from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import screen_search_cases as ssx

pytestmark = pytest.mark.gpu

NEED = 10      # the mixture's threshold: above the handful of chance 12-mers, far below any member
COUNTS = ("keys", "kmers", "entries", "slices", "query_keys", "lookups", "matched", "increments", "query_slices")
ROUNDS = ("entries", "rounds", "rows", "claimed", "decrements")


def _engine(genomes):
    from pyani_amd.engine import Engine
    e = Engine(0).__enter__()
    return e, [e.add_genome(s, o) for s, o in genomes]


@pytest.fixture(scope="module")
def fam():
    """(engine, ids of the 8 family genomes, ids of the 3 covered queries, ids of the 4 sparse queries)"""
    e, ids = _engine(list(scr.family()) + list(sac.covered_queries()) + list(sac.sparse_queries()))
    yield e, ids[:8], ids[8:11], ids[11:]
    e.__exit__(None, None, None)


def _count(e, queries, want, what=""):
    sizes, weight = e.screen_gather_count(queries, abundance=True)
    assert weight.dtype == np.uint64 and [int(x) for x in weight] == want.weight, (what, weight, want.weight)
    mw = e.screen_gather_abundance_matched()
    assert mw.dtype == np.uint64 and [int(x) for x in mw] == want.matched_weight, (what, mw, want.matched_weight)
    return sizes


def _result(e, want, rows, stats, sizes):
    from pyani_amd import screen
    q, n = want.gathered.hits.shape
    return screen.GatherResult([f"q{i}" for i in range(q)], [f"d{b}" for b in range(n)], screen.GatherOptions(16, 16, 1, abundance=True), sizes,
                               np.ones(n, np.uint32), *rows, want.gathered.matched, np.array(want.weight, np.uint64), e.screen_gather_abundance_matched(),
                               stats[0], screen.sumsq_words(stats[1]), *stats[2:])


def _device(e, want, need, sizes, max_ranks=65536, what=""):
    """One gather and one abundance pass over the counted queries, held to `want`: rows, every integer, the counters and the columns."""
    g = want.gathered
    q, n = g.hits.shape
    rows = e.screen_gather_rows(np.full(q, need, dtype=np.uint32) if np.isscalar(need) else need, max_ranks)
    sgc.same_rows(rows, g, what)
    stats = e.screen_gather_abundance()
    total, sumsq, median2, low, high = stats
    assert total.dtype == sumsq.dtype == median2.dtype == np.uint64 and low.dtype == high.dtype == np.uint32 and sumsq.shape == (len(g.query), 2), what
    print(what, "sum", total[:8], "sumsq", sumsq[:8].tolist(), "median2", median2[:8], "min", low[:8], "max", high[:8])
    assert [int(x) for x in total] == want.sum, (what, total, want.sum)
    assert [int(x) for x in sumsq[:, 0]] == [x & ((1 << 64) - 1) for x in want.sumsq] and [int(x) for x in sumsq[:, 1]] == [x >> 64 for x in want.sumsq], (what, sumsq)
    assert [int(x) for x in median2] == want.median2, (what, median2, want.median2)
    assert [int(x) for x in low] == want.min and [int(x) for x in high] == want.max, (what, low, high, want.min, want.max)
    last = e.screen_gather_abundance_last()
    got = {key: last[key] for key in ("attributed", "unattributed", "holders_walked", "rank_table_bytes")}
    assert got == {"attributed": int(g.unique.astype(np.int64).sum()), "unattributed": want.unattributed, "holders_walked": want.holders if len(g.query) else 0,
                   "rank_table_bytes": 4 * q * n if len(g.query) else 0}, (what, got)
    # what the plain calls give is what they gave without the abundances
    assert np.array_equal(e.screen_gather_fetch(), g.left) and np.array_equal(e.screen_gather_matched(), g.matched), what
    plain = e.screen_gather_last()
    assert {key: plain[key] for key in ROUNDS} == {"entries": int(g.matched.sum()), "rounds": g.rounds, "rows": len(g.query), "claimed": g.claimed,
                                                   "decrements": g.decrements}, (what, plain)
    # the float columns: the same expressions over the statement's integers
    r = _result(e, want, rows, stats, sizes)
    frame, summary = r.frame(), r.summary()
    for name, column in sac.columns(want).items():
        assert frame[name].tolist() == column, (what, name)
    for name, column in sac.summary_columns(want).items():
        assert [int(x) for x in summary[name]] == column, (what, name)
    return rows, stats


# ---- covered ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", scr.FAMILY_PARAMS)
def test_covered(fam, k, scale):
    e, db, queries, _ = fam
    want = sac.covered_expected(k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        sizes = _count(e, queries, want, ("covered", k, scale))
        assert (sizes == [len(scr.genome_set(s, o, k, scale)) for s, o in sac.covered_queries()]).all()
        rows, stats = _device(e, want, NEED, sizes, what=("covered", k, scale))
        first = int(np.flatnonzero((rows[0] == 0) & (rows[1] == 3))[0])
        assert stats[3][first] == 3      # genome 3 stands three times in the query: no k-mer of its row is held fewer times
        # another gather over the same count, every k-mer worth a row, and its pass: the entries and the abundances were left as the count made them
        _device(e, sac.covered_expected(k, scale, 1), 1, sizes, what=("covered, need 1", k, scale))
    finally:
        e.screen_search_index_release()


# ---- tiny, wide, many --------------------------------------------------------------------------------------------------------------------
def test_tiny():
    k, scale = sac.TINY_PARAMS
    db, query = sac.tiny()
    e, ids = _engine(list(db) + [query])
    want = sac.tiny_expected()
    try:
        e.screen_search_index(ids[:4], kmer=k, scale=scale)
        sizes = _count(e, ids[4:], want, "tiny")
        _, stats = _device(e, want, 1, sizes, what="tiny")
        assert stats[2].tolist() == [2, 2, 4, 10] and stats[0].tolist() == [4, 3, 4, 5]      # m = 4, 3, 2, 1: both parities, and the row of one k-mer
    finally:
        e.__exit__(None, None, None)


def test_wide():
    k, scale = scr.WIDE_PARAMS
    e, ids = _engine(list(scr.wide()) + [sac.wide_query()])
    want = sac.wide_expected()
    try:
        e.screen_search_index(ids[:scr.WIDE_N], kmer=k, scale=scale)
        sizes = _count(e, ids[scr.WIDE_N:], want, "wide")
        _device(e, want, 1, sizes, what="wide")
    finally:
        e.__exit__(None, None, None)


def test_many_ranks():
    k, scale = sgc.MANY_PARAMS
    e, ids = _engine(list(sgc.many()) + [sac.many_query()])
    full = sac.many_expected()
    assert full.min == [j % 5 + 1 for j in range(sgc.MANY_N - 1, -1, -1)]      # (a chance 16-mer of two members can only be held more often)
    try:
        db_sizes = e.screen_search_index(ids[:sgc.MANY_N], kmer=k, scale=scale)
        sizes = _count(e, ids[sgc.MANY_N:], full, "many")
        _device(e, full, 1, sizes, what="many")
        for max_ranks in (1, 7):      # the rows beyond max_ranks leave their entries to no row
            want = sac.many_expected(1, max_ranks)
            assert want.unattributed > 0
            _device(e, want, 1, sizes, max_ranks, what=("many", max_ranks))
        above = int(db_sizes.max()) + 1
        none = sac.many_expected(above)
        assert len(none.sum) == 0 and none.unattributed == int(full.gathered.matched.sum())
        _device(e, none, above, sizes, what="many, none")
    finally:
        e.__exit__(None, None, None)


# ---- slices: the abundances are appended in step with the entries ----------------------------------------------------------------------
def test_slices(fam):
    e, db, queries, _ = fam
    k, scale = 16, 16
    want = sac.covered_expected(k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        e.screen_gather_count(queries, abundance=True)
        one = e.screen_search_last()
        assert one["slices"] == one["query_slices"] == 1
        e.screen_set_budget(min(one["keys"], one["query_keys"]) // 3)
        e.screen_search_index(db, kmer=k, scale=scale)
        sizes = _count(e, queries, want, "slices")
        three = e.screen_search_last()
        assert three["slices"] >= 3 and three["query_slices"] >= 3 and three["query_keys"] == sum(want.weight)
        _device(e, want, NEED, sizes, what="slices")
    finally:
        e.screen_set_budget(0)
        e.screen_search_index_release()


# ---- entries that belong to no row -------------------------------------------------------------------------------------------------------
def test_unattributed_entries(fam):
    e, db, queries, _ = fam
    k, scale = 16, 16
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        for need, max_ranks in ((3800, 65536), (NEED, 1), (3800, 1)):      # above genome 7's 3763 k-mers; one row a query; both
            want = sac.covered_expected(k, scale, need, max_ranks)
            assert want.unattributed > 0 and any(u > 0 for u in sac.summary_columns(want)["unexplained_weight"])
            sizes = _count(e, queries, want, ("unattributed", need, max_ranks))
            _device(e, want, need, sizes, max_ranks, what=("unattributed", need, max_ranks))
    finally:
        e.screen_search_index_release()


# ---- queries without entries -------------------------------------------------------------------------------------------------------------
def test_queries_without_entries(fam):
    e, db, _, queries = fam
    k, scale = 16, 16
    want = sac.sparse_expected(k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        sizes = _count(e, queries, want, "sparse")
        assert sizes[2] == 0 and sizes[1] > 0
        rows, _ = _device(e, want, NEED, sizes, what="sparse")
        assert sorted(set(rows[0].tolist())) == [0, 3]
        # no query at all: no rows, nothing to read
        sizes, weight = e.screen_gather_count([], abundance=True)
        assert len(sizes) == 0 and len(weight) == 0 and len(e.screen_gather_abundance_matched()) == 0
        assert [len(x) for x in e.screen_gather_rows(np.zeros(0, np.uint32))] == [0, 0, 0, 0]
        assert [len(x) for x in e.screen_gather_abundance()] == [0, 0, 0, 0, 0]
        last = e.screen_gather_abundance_last()
        assert last["attributed"] == last["unattributed"] == last["holders_walked"] == last["rank_table_bytes"] == 0
    finally:
        e.screen_search_index_release()


# ---- what the abundance count leaves behind ------------------------------------------------------------------------------------------------
def test_the_abundance_count_leaves_what_the_plain_count_leaves(fam):
    e, db, queries, _ = fam
    k, scale = 12, 16
    need = np.full(3, NEED, np.uint32)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        seen = []
        for abundance in (False, True):
            sizes = e.screen_gather_count(queries, abundance=abundance)
            sizes = sizes[0] if abundance else sizes
            search = e.screen_search_last()
            rect = e.screen_search_fetch()
            rows = e.screen_gather_rows(need)
            if abundance:
                e.screen_gather_abundance()
            rounds = e.screen_gather_last()
            seen.append((sizes, rect, e.screen_gather_fetch(), e.screen_gather_matched(), *rows, [search[c] for c in COUNTS], [rounds[c] for c in ROUNDS]))
        for plain, weighted in zip(*seen):
            assert np.array_equal(plain, weighted)
        assert len(seen[0][4]) > 0
    finally:
        e.screen_search_index_release()


# ---- the order of the calls --------------------------------------------------------------------------------------------------------------
def test_order_of_calls(fam):
    from pyani_amd import screen
    e, db, queries, _ = fam
    k, scale = 16, 16
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        want = sac.covered_expected(k, scale, NEED)
        sizes = _count(e, queries, want, "order")
        before = e.screen_search_fetch()
        _device(e, want, NEED, sizes, what="order, first")
        other = sac.covered_expected(k, scale, 2000, 1)
        assert other.sum != want.sum
        _device(e, other, 2000, sizes, 1, what="order, other thresholds")
        _device(e, want, NEED, sizes, what="order, the first again")
        assert np.array_equal(e.screen_search_fetch(), before) and np.array_equal(before, want.gathered.hits)
        dsizes = scr.expected("family", k, scale)[0]
        need_q, need_db = screen.identity_thresholds(sizes, k, 0.8, 2), screen.identity_thresholds(dsizes, k, 0.8, 2)
        ssx.same(e.screen_search_select(need_q, need_db), ssx.rule_block(want.gathered.hits, need_q, need_db), "select after the abundances")
    finally:
        e.screen_search_index_release()


# ---- chunks ------------------------------------------------------------------------------------------------------------------------------
def test_chunks(fam, monkeypatch):
    from pyani_amd import screen
    e, db, queries, sparse = fam
    k, scale = 16, 16
    ids = list(queries) + list(sparse)
    genomes = list(sac.covered_queries()) + list(sac.sparse_queries())
    want = sac.abundance_genomes(genomes, scr.family(), k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        monkeypatch.setattr(e, "_band_rows", 2, raising=False)      # chunks of 2, 2, 2 and 1 queries
        r = e.screen_gather(ids, screen.GatherOptions(k, scale, NEED, abundance=True))
        sgc.same_rows((r.query, r.db, r.unique, r.total), want.gathered, "chunks")
        assert [int(x) for x in r.query_weight] == want.weight and [int(x) for x in r.matched_weight] == want.matched_weight
        assert [int(x) for x in r.sum_abund] == want.sum and r.sumsq_abund.tolist() == want.sumsq and [int(x) for x in r.median2_abund] == want.median2
        assert [int(x) for x in r.min_abund] == want.min and [int(x) for x in r.max_abund] == want.max
        frame = r.frame()
        for name, column in sac.columns(want).items():
            assert frame[name].tolist() == column, name
        plain = e.screen_gather(ids, screen.GatherOptions(k, scale, NEED))
        assert not plain.has_abundance() and plain.frame().equals(frame[list(plain.frame().columns)])
    finally:
        e.screen_search_index_release()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(fam):
    from pyani_amd import _lib
    e, db, queries, _ = fam
    k, scale = 16, 16
    want = sac.covered_expected(k, scale, NEED)
    need = np.full(3, NEED, np.uint32)

    def refused(call, message):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and message in str(err.value), str(err.value)

    def still_readable():
        r = len(want.sum)
        out = [np.zeros(r, np.uint64), np.zeros(2 * r, np.uint64), np.zeros(r, np.uint64), np.zeros(r, np.uint32), np.zeros(r, np.uint32)]
        assert e.lib.pg_screen_gather_abund_read(e._h, *(ctypes.c_void_p(x.ctypes.data) for x in out)) == 0
        assert [int(x) for x in out[0]] == want.sum and [int(x) for x in out[2]] == want.median2 and [int(x) for x in out[4]] == want.max
        assert [int(x) for x in e.screen_gather_abundance_matched()] == want.matched_weight

    e.screen_search_index_release()
    refused(lambda: e.screen_gather_abundance(), "no resident search index")
    refused(lambda: e.screen_gather_abundance_matched(), "kept no abundances")
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        refused(lambda: e.screen_gather_abundance(), "kept no abundances")
        e.screen_gather_count(queries)      # the plain count keeps the entries, not the abundances
        e.screen_gather_rows(need)
        refused(lambda: e.screen_gather_abundance(), "kept no abundances")
        refused(lambda: e.screen_gather_abundance_matched(), "kept no abundances")
        sizes = _count(e, queries, want, "refusals")
        refused(lambda: e.screen_gather_abundance(), "no gathered rows since that count")
        assert e.lib.pg_screen_gather_abund_read(e._h, None, None, None, None, None) == _lib.PG_E_ARG      # no pass yet
        _device(e, want, NEED, sizes, what="before the refusals")
        assert e.lib.pg_screen_gather_abund(e._h, None) == _lib.PG_E_ARG
        still_readable()
        assert e.lib.pg_screen_gather_abund_read(e._h, None, None, None, None, None) == _lib.PG_E_ARG      # rows, and nowhere to put them
        still_readable()
        refused(lambda: e.screen_gather_rows(need[:2]), "3 queries, not 2")      # a refused gather leaves the statistics of the one before
        still_readable()
        e.screen_gather_rows(need)      # a new gather: its statistics are not made yet
        assert e.lib.pg_screen_gather_abund_read(e._h, None, None, None, None, None) == _lib.PG_E_ARG
        assert "no abundance statistics" in e.lib.pg_last_error(e._h).decode()
        e.screen_gather_abundance()
        still_readable()
        # a plain count drops the abundances with the entries
        e.screen_search_count(queries)
        refused(lambda: e.screen_gather_abundance_matched(), "kept no abundances")
        assert e.screen_gather_abundance_last()["attributed"] == 0
    finally:
        e.screen_search_index_release()


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    import pandas as pd
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_gather import run_screen_gather
    from pyani_amd.subcmd_searchdb import run_screen_index_build
    k, scale = 16, 16
    db_dir, q_dir = tmp_path / "db", tmp_path / "queries"
    db_dir.mkdir(), q_dir.mkdir()
    for g, (seq, off) in enumerate(scr.family()):
        synth.write_fasta(db_dir / f"fam{g}.fna", seq, off, f"fam{g}")
    queries = sac.covered_queries()
    for name, (seq, off) in zip(("mix", "copy"), queries):
        synth.write_fasta(q_dir / f"{name}.fna", seq, off, name)
    want = sac.abundance_genomes([queries[1], queries[0]], scr.family(), k, scale, NEED)      # file order: copy.fna, mix.fna
    rows_columns = ["query", "rank", "db", "unique", "total", "f_unique_query", "f_unique_cumulative", "f_match", "identity"]
    summary_columns = ["query", "size", "matched", "rows", "explained", "unexplained"]
    with Engine(0) as eng:
        run_screen_index_build(db_dir, tmp_path / "family.idx", kmer=k, scale=scale, engine=eng)
        plain = run_screen_gather(db_dir, q_dir, tmp_path / "plain", min_unique=NEED, kmer=k, scale=scale, write_output=True, engine=eng)
        assert list(plain.frame.columns) == rows_columns and list(plain.summary.columns) == summary_columns and not plain.result.has_abundance()
        tables = []
        for where, source in (("from_dir", {"db_dir": db_dir}), ("from_index", {"db_dir": None, "index": tmp_path / "family.idx"})):
            run = run_screen_gather(query_dir=q_dir, outdir=tmp_path / where, min_unique=NEED, kmer=k, scale=scale, write_output=True, engine=eng, abundance=True, **source)
            assert eng.genome_count() == 0 and eng._search is None
            r = run.result
            sgc.same_rows((r.query, r.db, r.unique, r.total), want.gathered, where)
            assert [int(x) for x in r.sum_abund] == want.sum and r.sumsq_abund.tolist() == want.sumsq and [int(x) for x in r.query_weight] == want.weight
            rows_tab, summary_tab = (pd.read_csv(p, sep="\t", float_precision="round_trip") for p in run.written)
            assert list(rows_tab.columns) == rows_columns + list(sac.columns(want)) and list(summary_tab.columns) == summary_columns + list(sac.summary_columns(want))
            for name, column in sac.columns(want).items():
                assert rows_tab[name].tolist() == column, (where, name)
            for name, column in sac.summary_columns(want).items():
                assert summary_tab[name].tolist() == column, (where, name)
            assert list(zip(rows_tab["query"], rows_tab["db"])) == [("copy", "fam0"), ("mix", "fam3"), ("mix", "fam7")]
            assert rows_tab["median_abund"].tolist() == [1.0, 3.0, 1.0]      # genome 3 three times, genome 7 once
            assert rows_tab[rows_columns].equals(pd.read_csv(plain.written[0], sep="\t", float_precision="round_trip"))
            tables.append([p.read_bytes() for p in run.written])
        assert tables[0] == tables[1]
        # exact="anim" beside the abundances: its two columns come last
        exact = run_screen_gather(db_dir, q_dir, min_unique=NEED, kmer=k, scale=scale, exact="anim", engine=eng, abundance=True)
        assert list(exact.frame.columns) == rows_columns + list(sac.columns(want)) + ["anim_identity", "anim_coverage_db"] and (exact.frame["anim_identity"] > 0.999).all()
