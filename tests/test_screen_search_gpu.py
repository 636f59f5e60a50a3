"""GPU (through the C ABI): the screen's search (pg_screen_search_index / _count / _select / _read / _fetch / _last / _index_release;
pyani_amd/csrc/pgscr_search.inc) against blocks of the numpy statement of the screen (tests/screen_cases.py) and the
numpy statement of the rule on a rectangle (tests/screen_search_cases.py).  Everything is an integer and must be EQUAL: the rectangle,
the sizes, the counters and every selection, in the same order — whatever the chunks of queries, the slices of the index, the slices
of the queries or what became of the genome store after the index was built."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_index_cases as sic
from tests import screen_search_cases as ssx
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu


def _rect_equals(e, want, what):
    got = e.screen_search_fetch()
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def _distinct_kmers(case, k, scale, genomes):
    return len(np.unique(np.concatenate([scr.genome_set(*scr.CASES[case]()[g], k, scale) for g in genomes])))


@pytest.fixture(scope="module")
def small_engines():
    """{case: (engine, ids)} for family and edges: the genomes loaded once."""
    from pyani_amd.engine import Engine
    out, open_ = {}, []
    for case in ("family", "edges"):
        e = Engine(0).__enter__()
        open_.append(e)
        out[case] = (e, [e.add_genome(s, o) for s, o in scr.CASES[case]()])
    yield out
    for e in open_:
        e.__exit__(None, None, None)


def _selections(e, case, k, scale, queries, db, kept):
    """Every threshold x min_shared on the resident rectangle; returns the kept counts at min_shared = 2."""
    from pyani_amd import screen
    qs, ds, hits = ssx.block(case, k, scale, queries, db)
    sizes, shared = scr.expected(case, k, scale)
    counts = []
    for t in ssc.THRESHOLDS:
        for ms in (1, 2):
            need_q, need_db = screen.identity_thresholds(qs, k, t, ms), screen.identity_thresholds(ds, k, t, ms)
            got = e.screen_search_select(need_q, need_db)
            ssx.same(got, ssx.rule_block(hits, need_q, need_db), (case, k, scale, t, ms))
            ssx.same(got, ssx.restricted(shared, screen.identity_thresholds(sizes, k, t, ms), queries, db), (case, k, scale, t, ms, "all-vs-all"))
            if ms == 2:
                counts.append(len(got[0]))
    if kept is not None:
        assert tuple(counts) == kept
    return counts


# ---- family ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", scr.FAMILY_PARAMS)
def test_family(small_engines, k, scale):
    e, ids = small_engines["family"]
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    qs, ds, hits = ssx.block("family", k, scale, queries, db)
    try:
        sizes = e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale)
        assert sizes.dtype == np.uint32 and (sizes == ds).all(), (sizes, ds)
        qsizes = e.screen_search_count([ids[g] for g in queries])
        assert qsizes.dtype == np.uint32 and (qsizes == qs).all(), (qsizes, qs)
        _rect_equals(e, hits, ("family", k, scale))
        assert hits[3, 4] == qs[3] == ds[4] > 0      # genome 7 meets itself: the no-diagonal cell
        last = e.screen_search_last()
        assert last["increments"] == int(hits.astype(np.int64).sum())
        assert last["lookups"] == _distinct_kmers("family", k, scale, queries)
        assert last["kmers"] == _distinct_kmers("family", k, scale, db) and last["entries"] == int(ds.sum())
        assert last["keys"] >= last["entries"] and last["query_keys"] >= int(qs.sum()) and last["slices"] == last["query_slices"] == 1
        assert 0 < last["matched"] <= min(last["lookups"], last["kmers"])
        counts = _selections(e, "family", k, scale, queries, db, ssx.FAMILY_KEPT.get((k, scale)))
        assert counts[0] == 20 and counts[-1] == 3 and ((k, scale) not in ssx.FAMILY_KEPT or 3 < counts[3] < 20)      # all, some and few
        # the three: the two exact copies against the ancestor, and genome 7 with itself
        a, b, s = e.screen_search_select(*(np.asarray(x) for x in _needs(qs, ds, k, 1.0, 2)))
        assert list(zip(a.tolist(), b.tolist())) == [(0, 0), (1, 0), (3, 4)] and (s == [ds[0], ds[0], ds[4]]).all()
    finally:
        e.screen_search_index_release()


def _needs(qs, ds, k, t, ms):
    from pyani_amd import screen
    return screen.identity_thresholds(qs, k, t, ms), screen.identity_thresholds(ds, k, t, ms)


# ---- the index's memory ----------------------------------------------------------------------------------------------------------------------
def test_the_index_moves_into_blocks_of_its_own_size(small_engines):
    """The arrays are allocated by the bound (keys) and moved afterwards: index_bytes is what the buffers HOLD.  On family D is about three
    quarters of the keys — four of the five db genomes are related and share k-mers — so the values and the starts must have moved; the
    members move only when E is more than a sixteenth below the keys.  The search over the moved arrays gives the statement's rectangle."""
    e, ids = small_engines["family"]
    k, scale = 16, 16
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    qs, ds, hits = ssx.block("family", k, scale, queries, db)
    try:
        for budget in (0, None):      # one slice; three or more
            if budget is None:
                budget = e.screen_search_last()["keys"] // 3
            e.screen_set_budget(budget)
            e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale)
            last = e.screen_search_last()
            keys, d, ent = last["keys"], last["kmers"], last["entries"]

            def held(need):      # the rule of the move: exact unless the bound was within a sixteenth
                return need if keys + 1 > need + need // 16 + 64 else None
            assert ent == int(ds.sum()) and held(d + 1) == d + 1      # the design: the values and the starts must move
            directory = 8 * (last["slices"] + 1) + 4 * scr.N_BINS
            members = held(ent + 1) or keys + 1
            assert last["index_bytes"] == 4 * (d + 1) + 8 * (d + 1) + 4 * members + directory
            assert last["index_bytes"] < 16 * (keys + 1)      # under what the build allocated, the directory included
            assert (e.screen_search_count([ids[g] for g in queries]) == qs).all()
            _rect_equals(e, hits, ("moved", budget))
    finally:
        e.screen_set_budget(0)
        e.screen_search_index_release()
    assert e.screen_search_last()["index_bytes"] == 0


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
def test_edges(small_engines):
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    queries, db = ssx.EDGES_QUERIES, ssx.EDGES_DB
    qs, ds, hits = ssx.block("edges", k, scale, queries, db)
    assert qs[0] == qs[1] == 0 and (hits[:2] == 0).all() and hits[2, 0] == ds[0] and hits[3, 1] == ds[1]
    try:
        assert (e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale) == ds).all()
        assert (e.screen_search_count([ids[g] for g in queries]) == qs).all()
        _rect_equals(e, hits, "edges")
        last = e.screen_search_last()
        assert last["increments"] == int(hits.astype(np.int64).sum()) and last["lookups"] == _distinct_kmers("edges", k, scale, queries)
        _selections(e, "edges", k, scale, queries, db, ssx.EDGES_KEPT)
        a, b, s = e.screen_search_select(np.zeros(4, np.uint32), np.zeros(3, np.uint32))      # threshold 0: the empty queries keep their zero cells
        assert len(a) == 12 and (s[:6] == 0).all() and a[:6].tolist() == [0, 0, 0, 1, 1, 1]
    finally:
        e.screen_search_index_release()


# ---- chunks and slices ---------------------------------------------------------------------------------------------------------------------
def test_chunks_and_slices_change_nothing(small_engines):
    from pyani_amd import _lib, screen
    e, ids = small_engines["family"]
    k, scale = 16, 16
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    qs, ds, hits = ssx.block("family", k, scale, queries, db)
    q_ids, db_ids = [ids[g] for g in queries], [ids[g] for g in db]
    opt = screen.ScreenOptions(0.8, k, scale, 2)
    want = ssx.rule_block(hits, *_needs(qs, ds, k, 0.8, 2))
    assert 0 < len(want[0]) < hits.size
    try:
        e.screen_search_index(db_ids, kmer=k, scale=scale)
        one = e.screen_search_last()
        e.screen_search_count(q_ids)
        query_keys = e.screen_search_last()["query_keys"]
        assert one["slices"] == 1
        for index_budget, query_budget in ((0, 0), (one["keys"] // 3, 0), (0, query_keys // 3), (one["keys"] // 3, query_keys // 3)):
            e.screen_set_budget(index_budget)
            e.screen_search_index(db_ids, kmer=k, scale=scale)
            built = e.screen_search_last()
            assert (built["slices"] > 1) == bool(index_budget)
            assert {x: built[x] for x in ("keys", "kmers", "entries")} == {x: one[x] for x in ("keys", "kmers", "entries")}
            e.screen_set_budget(query_budget)
            for band in (1, 3, 0):
                e.screen_set_band(band)
                got = e.screen_search(q_ids, opt)
                assert (got.query_sizes == qs).all() and (got.db_sizes == ds).all()
                ssx.same((got.a, got.b, got.shared), want, (index_budget, query_budget, band))
                last = e.screen_search_last()      # of the last chunk
                rows = {1: 1, 3: 1, 0: 4}[band]      # 4 queries: four chunks of 1; 3 + 1; one of 4
                if band == 0:      # (a chunk of one query has a quarter of the keys: it fits the budget in one slice)
                    assert (last["query_slices"] > 1) == bool(query_budget)
                _rect_equals(e, hits[4 - rows:], (index_budget, query_budget, band))
                assert last["increments"] == int(hits[4 - rows:].astype(np.int64).sum())
                if band:      # more queries than the band's rows
                    with pytest.raises(_lib.PyaniGpuError, match="band"):
                        e.screen_search_count(q_ids)
    finally:
        e.screen_set_budget(0)
        e.screen_set_band(0)
        e.screen_search_index_release()


# ---- wide groups ---------------------------------------------------------------------------------------------------------------------------
def test_wide_groups():
    from pyani_amd.engine import Engine
    k, scale = scr.WIDE_PARAMS
    n, split = scr.WIDE_N, scr.WIDE_N - 10
    want_sizes, want_shared = scr.expected("wide", k, scale)
    queries, db = list(range(split, n)), list(range(split))
    hits = want_shared[split:, :split]
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in scr.wide()]
        assert (e.screen_search_index(ids[:split], kmer=k, scale=scale) == want_sizes[:split]).all()
        assert (e.screen_search_count(ids[split:]) == want_sizes[split:]).all()
        _rect_equals(e, hits, "wide")
        last = e.screen_search_last()
        assert last["increments"] == int(hits.astype(np.int64).sum()) >= 9 * 10 * split      # motif 1: nine k-mers of 2990 holders, ten queries each
        # the corner: genome 2999 shares motif 2 with genome 0 alone
        base = int(np.bincount(hits.reshape(-1).astype(np.int64)).argmax())
        assert hits[9, 0] > base + 1
        need_q, need_db = np.full(10, hits[9, 0], np.uint32), np.full(split, hits[9, 0], np.uint32)
        got = e.screen_search_select(need_q, need_db)
        ssx.same(got, ssx.rule_block(hits, need_q, need_db), "wide")
        assert ((got[0] == 9) & (got[1] == 0)).any() and 0 < len(got[0]) < hits.size // 2      # (the bulk shares motif 1 alone and is dropped)
        assert not ((got[0] == 0) & (got[1] == 2)).any()      # genomes 2990 and 2: motif 1 alone


# ---- beyond 8192 ---------------------------------------------------------------------------------------------------------------------------
def test_beyond_8192_db_genomes():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    split, n = 8196, sic.BEYOND_N
    hits = sic.beyond_rows(split, n)[:, :split]
    t = sic.beyond_threshold()[0]
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        assert (e.screen_search_index(ids[:split], kmer=k, scale=scale) == sic.beyond_sizes()[:split]).all()
        assert (e.screen_search_count(ids[split:]) == sic.beyond_sizes()[split:]).all()
        _rect_equals(e, hits, "beyond")
        got = e.screen_search(ids[split:], screen.ScreenOptions(t, k, scale))
        assert got.pairs() == [(3, 0), (3, 8191), (3, 8192)]      # query 8199 and the three other B holders; the other queries keep nothing
        assert (got.shared == hits[3, [0, 8191, 8192]]).all()


# ---- lifetime ------------------------------------------------------------------------------------------------------------------------------
def test_the_index_outlives_the_genome_store():
    from pyani_amd import _lib, screen
    from pyani_amd.engine import Engine
    k, scale = 16, 16
    genomes = scr.family()
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    qs, ds, hits = ssx.block("family", k, scale, queries, db)
    opt = screen.ScreenOptions(0.8, k, scale, 2)
    with Engine(0) as e:
        both = [e.add_genome(s, o) for s, o in genomes]
        e.screen_search_index([both[g] for g in db], kmer=k, scale=scale)
        before = e.screen_search([both[g] for g in queries], opt)
        e.screen_search_index_release()
        e.clear_genomes()
        e.screen_search_index([e.add_genome(*genomes[g]) for g in db], kmer=k, scale=scale)
        e.clear_genomes()
        assert e.genome_count() == 0
        q_ids = [e.add_genome(*genomes[g]) for g in queries]      # only the queries: they take the collection's place in the store
        after = e.screen_search(q_ids, opt)
        _rect_equals(e, hits, "after clear_genomes")
        ssx.same((after.a, after.b, after.shared), (before.a, before.b, before.shared), "after clear_genomes")
        ssx.same((after.a, after.b, after.shared), ssx.rule_block(hits, *_needs(qs, ds, k, 0.8, 2)), "after clear_genomes")
        assert (after.db_sizes == ds).all() and (after.query_sizes == qs).all() and 0 < len(after.a) < hits.size
        e.screen_search_index_release()
        e.screen_search_index_release()      # nothing resident: still fine
        with pytest.raises(_lib.PyaniGpuError, match="no resident search index"):
            e.screen_search_count(q_ids)


# ---- the existing path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale,queries,db", [("family", 16, 16, ssx.FAMILY_QUERIES[:3], ssx.FAMILY_DB),
                                                     ("edges", *scr.EDGES_PARAMS, ssx.EDGES_QUERIES[:3], ssx.EDGES_DB)])
def test_search_equals_the_rows_of_screen_candidates(small_engines, case, k, scale, queries, db):
    from pyani_amd import screen
    e, ids = small_engines[case]      # (disjoint queries and db: screen_candidates takes no genome twice)
    union = db + queries
    lengths = set()
    try:
        e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale, labels=[f"g{g}" for g in db])
        for t in ssc.THRESHOLDS:
            opt = screen.ScreenOptions(t, k, scale, 2)
            got = e.screen_search([ids[g] for g in queries], opt, query_labels=[f"g{g}" for g in queries])
            sp = e.screen_candidates([ids[g] for g in union], opt, path="index")
            rows = (sp.a >= len(db)) & (sp.b < len(db))
            ssx.same((got.a, got.b, got.shared), (sp.a[rows] - np.int32(len(db)), sp.b[rows], sp.shared[rows]), (case, t))
            assert (got.query_sizes == sp.sizes[len(db):]).all() and (got.db_sizes == sp.sizes[:len(db)]).all()
            assert got.query_labels == [f"g{g}" for g in queries] and got.db_labels == [f"g{g}" for g in db] and got.options == opt
            lengths.add(len(got.a))
        assert max(lengths) == len(queries) * len(db) and len(lengths) >= 2
    finally:
        e.screen_search_index_release()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_and_the_rectangle_readable(small_engines):
    from pyani_amd import _lib, screen
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    queries, db = ssx.EDGES_QUERIES, ssx.EDGES_DB
    qs, ds, hits = ssx.block("edges", k, scale, queries, db)
    q_ids, db_ids = [ids[g] for g in queries], [ids[g] for g in db]
    need_q, need_db = np.full(4, 2, np.uint32), np.full(3, 2, np.uint32)
    want = ssx.rule_block(hits, need_q, need_db)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    e.screen_search_index_release()
    refused(lambda: e.screen_search_count(q_ids), "no resident search index")
    refused(lambda: e.screen_search_select(need_q, need_db), "no resident search index")
    refused(lambda: e.screen_search_fetch(), "no resident search index")
    refused(lambda: e._check(e.lib.pg_screen_search_read(e._h, None, None, None)), "no selection")
    assert e.screen_search_last()["kmers"] == 0
    with pytest.raises(ValueError, match="no search index"):
        e.screen_search(q_ids, 0.8)
    try:
        assert (e.screen_search_index(db_ids, kmer=k, scale=scale) == ds).all()
        refused(lambda: e.screen_search_select(need_q, need_db), "no counted rectangle")
        refused(lambda: e.screen_search_fetch(), "no counted rectangle")
        refused(lambda: e._check(e.lib.pg_screen_search_read(e._h, None, None, None)), "no selection")
        assert (e.screen_search_count(q_ids) == qs).all()
        ssx.same(e.screen_search_select(need_q, need_db), want, "before the refusals")

        def still_there(what):
            _rect_equals(e, hits, what)
            ssx.same(e.screen_search_select(need_q, need_db), want, what)
        refused(lambda: e.screen_search_select(need_q[:3], need_db), "not 3")
        refused(lambda: e.screen_search_select(need_q, need_db[:2]), "not 2")
        refused(lambda: e.screen_search_select(need_q, np.zeros(4, np.uint32)), "not 4")
        refused(lambda: e._check(e.lib.pg_screen_search_select(e._h, None, 4, need_db.ctypes.data, 3, None)), "bad argument")
        still_there("after refused selections")
        refused(lambda: e.screen_search_count([q_ids[0], q_ids[1], q_ids[0]]), "twice")
        refused(lambda: e.screen_search_count([q_ids[0], 10 ** 6]), "out of range")
        refused(lambda: e.screen_search_count([-1]), "out of range")
        refused(lambda: e._check(e.lib.pg_screen_search_count(e._h, None, 2, None)), "bad argument")
        e.screen_set_band(3)
        refused(lambda: e.screen_search_count(q_ids), "band")
        e.screen_set_band(0)
        still_there("after refused counts")
    finally:
        e.screen_set_band(0)
    try:
        refused(lambda: e.screen_search_index([db_ids[0], db_ids[0]], kmer=k, scale=scale), "twice")
        refused(lambda: e.screen_search_index(db_ids, kmer=7, scale=scale), "8 ... 16")
        refused(lambda: e.screen_search_index(db_ids, kmer=k, scale=3), "power of two")
        refused(lambda: e.screen_search_index(list(range(2 ** 20 + 1)), kmer=k, scale=scale), "2^20")
        still_there("after refused builds")
        with pytest.raises(ValueError, match="kmer"):
            e.screen_search(q_ids, screen.ScreenOptions(0.8, 12, scale))
        # the other resident states do not touch this one, nor it them
        sizes70, loaded = ssc.random_symmetric(13, 70)
        e.screen_load(loaded)
        e.screen_index(db_ids, kmer=k, scale=scale)
        e.screen_index_select(need_db)
        e.screen_index_release()
        still_there("after a load and an index")
        assert (e.screen_fetch() == loaded).all()
        e.screen_release()
    finally:
        e.screen_search_index_release()
