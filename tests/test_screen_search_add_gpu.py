"""GPU (through the C ABI): genomes ADDED to the resident search index (pg_screen_search_index_add / pg_screen_search_add_last;
pyani_amd/csrc/pgscr_add.inc).  An index built from a list and grown by adds must be the index a fresh build over the
whole list leaves: the statements are the ones of the search and the gather (tests/screen_cases.py, screen_search_cases.py,
screen_index_cases.py, screen_gather_cases.py), everything is an integer and must be EQUAL — the rectangle, the sizes, the counters,
every selection and every gathered row, in the same order — however the list was split, however the index and the batch were sliced,
and whatever became of the genome store between the batches."""
import functools

import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import screen_index_cases as sic
from tests import screen_search_cases as ssx
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

ALL8 = list(range(8))


def _rect_equals(e, want, what):
    got = e.screen_search_fetch()
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _distinct(case, k, scale, genomes):
    sets = [scr.genome_set(*scr.CASES[case]()[g], k, scale) for g in genomes]
    return len(np.unique(np.concatenate(sets))) if sets else 0


def _needs(qs, ds, k, t, ms):
    from pyani_amd import screen
    return screen.identity_thresholds(qs, k, t, ms), screen.identity_thresholds(ds, k, t, ms)


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


def _grow(e, ids, case, k, scale, parts):
    """index(parts[0]), add(parts[1]), ...: the sizes and the add's counters of every step held to the statement."""
    sizes = scr.expected(case, k, scale)[0]
    got = e.screen_search_index([ids[g] for g in parts[0]], kmer=k, scale=scale)
    assert got.dtype == np.uint32 and (got == sizes[parts[0]]).all(), (got, sizes[parts[0]])
    assert e.screen_search_add_last() == dict.fromkeys(e.screen_search_add_last(), 0)      # a build: nothing added yet
    keys, merged = e.screen_search_last()["keys"], False
    for i, part in enumerate(parts[1:]):
        got = e.screen_search_index_add([ids[g] for g in part])
        assert got.dtype == np.uint32 and (got == sizes[part]).all(), (part, got, sizes[part])
        add = e.screen_search_add_last()
        assert add["genomes"] == len(part) and add["adds"] == i + 1
        assert add["entries"] == int(sizes[part].sum()) and add["keys"] >= add["entries"]
        assert add["new_kmers"] + add["matched_kmers"] == _distinct(case, k, scale, tuple(part)), (part, add)
        before = sum((list(p) for p in parts[:i + 1]), [])
        assert add["new_kmers"] == _distinct(case, k, scale, tuple(before + list(part))) - _distinct(case, k, scale, tuple(before)), (part, add)
        keys += add["keys"]
        merged = merged or add["entries"] > 0
    whole = sum((list(p) for p in parts), [])
    last = e.screen_search_last()
    assert last["keys"] == keys and last["kmers"] == _distinct(case, k, scale, tuple(whole)) and last["entries"] == int(sizes[whole].sum()), last
    if merged:      # what the buffers hold after a merge: the exact sizes, and the directory
        assert last["index_bytes"] == 12 * (last["kmers"] + 1) + 4 * (last["entries"] + 1) + 8 * (last["slices"] + 1) + 4 * scr.N_BINS, last
    return last


# ---- 1. family: the added index is the fresh one -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", scr.FAMILY_PARAMS)
def test_family(small_engines, k, scale):
    e, ids = small_engines["family"]
    qs, ds, hits = ssx.block("family", k, scale, ALL8, ALL8)
    assert (np.diag(hits) == qs).all() and (qs == ds).all()      # the whole matrix, the sizes on the diagonal
    try:
        for parts in ([[0], ALL8[1:]], [ALL8[:4], ALL8[4:]], [ALL8[:7], [7]], [[0], [1, 2, 3], [4, 5, 6, 7]]):
            _grow(e, ids, "family", k, scale, parts)
            assert (e.screen_search_count([ids[g] for g in ALL8]) == qs).all()
            _rect_equals(e, hits, ("family", k, scale, parts))
            assert e.screen_search_last()["increments"] == int(hits.astype(np.int64).sum())
            for t in ssc.THRESHOLDS:
                for ms in (1, 2):
                    need_q, need_db = _needs(qs, ds, k, t, ms)
                    ssx.same(e.screen_search_select(need_q, need_db), ssx.rule_block(hits, need_q, need_db), (k, scale, parts, t, ms))
    finally:
        e.screen_search_index_release()


# ---- 2. slices change nothing --------------------------------------------------------------------------------------------------------------
def test_slices_change_nothing(small_engines):
    e, ids = small_engines["family"]
    k, scale = 16, 16
    first, rest = ALL8[:4], ALL8[4:]
    qs, ds, hits = ssx.block("family", k, scale, ALL8, ALL8)
    try:
        one = _grow(e, ids, "family", k, scale, [first, rest])
        index_keys, batch_keys = one["keys"] - e.screen_search_add_last()["keys"], e.screen_search_add_last()["keys"]
        assert one["slices"] == 1
        for index_budget in (index_keys // 3, 0):
            for add_budget in (0, batch_keys // 3):
                e.screen_set_budget(index_budget)
                e.screen_search_index([ids[g] for g in first], kmer=k, scale=scale)
                built = e.screen_search_last()["slices"]
                assert (built >= 3) == bool(index_budget)
                e.screen_set_budget(add_budget)
                e.screen_search_index_add([ids[g] for g in rest])
                add, last = e.screen_search_add_last(), e.screen_search_last()
                assert last["slices"] == built      # the merged directory is the index's
                assert {x: last[x] for x in ("keys", "kmers", "entries")} == {x: one[x] for x in ("keys", "kmers", "entries")}
                assert add["new_kmers"] + add["matched_kmers"] == _distinct("family", k, scale, tuple(rest)) and add["entries"] == int(ds[rest].sum())
                e.screen_set_budget(0)
                assert (e.screen_search_count([ids[g] for g in ALL8]) == qs).all()
                _rect_equals(e, hits, (index_budget, add_budget))
    finally:
        e.screen_set_budget(0)
        e.screen_search_index_release()


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges(small_engines):
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    sizes, shared = scr.expected("edges", k, scale)
    everyone = list(range(6))
    assert sizes[2] == sizes[3] == 0 and sizes[4] == sizes[0] > 0
    try:
        # an index without a slice: neither genome has a k-mer; the batch brings the directory
        _grow(e, ids, "edges", k, scale, [[2, 3], [0, 1, 5]])
        assert e.screen_search_last()["slices"] >= 1 and e.screen_search_add_last()["matched_kmers"] == 0
        assert (e.screen_search_count([ids[g] for g in everyone]) == sizes).all()
        _rect_equals(e, shared[np.ix_(everyone, [2, 3, 0, 1, 5])], "a slice-less index grows")
        # the empty genomes join a full index: two columns of zeros, and not an entry moves
        full = _grow(e, ids, "edges", k, scale, [[0, 1, 5]])
        last = _grow(e, ids, "edges", k, scale, [[0, 1, 5], [2, 3]])
        assert {x: last[x] for x in ("kmers", "entries", "slices", "index_bytes")} == {x: full[x] for x in ("kmers", "entries", "slices", "index_bytes")}
        add = e.screen_search_add_last()
        assert (add["entries"], add["new_kmers"], add["matched_kmers"], add["genomes"]) == (0, 0, 0, 2)
        e.screen_search_count([ids[g] for g in everyone])
        want = shared[np.ix_(everyone, [0, 1, 5, 2, 3])]
        assert (want[:, 3:] == 0).all()
        _rect_equals(e, want, "empty genomes join")
        # the twin of genome 0: every k-mer of it is there already
        _grow(e, ids, "edges", k, scale, [[0, 1, 5], [4]])
        add = e.screen_search_add_last()
        assert add["matched_kmers"] == _distinct("edges", k, scale, (4,)) == sizes[4] and add["new_kmers"] == 0
        e.screen_search_count([ids[g] for g in everyone])
        _rect_equals(e, shared[np.ix_(everyone, [0, 1, 5, 4])], "the twin joins")
        # genome 0 in two adds: the ids are not compared with the collection, the columns are equal
        e.screen_search_index([ids[1], ids[5]], kmer=k, scale=scale)
        for _ in range(2):
            assert (e.screen_search_index_add([ids[0]]) == sizes[[0]]).all()
        assert e.screen_search_add_last()["adds"] == 2 and e.screen_search_add_last()["new_kmers"] == 0
        e.screen_search_count([ids[g] for g in everyone])
        _rect_equals(e, shared[np.ix_(everyone, [1, 5, 0, 0])], "one genome twice")
    finally:
        e.screen_search_index_release()


# ---- 4. wide: groups of 2990 holders grow ------------------------------------------------------------------------------------------------------
def test_wide_groups_grow():
    from pyani_amd.engine import Engine
    k, scale = scr.WIDE_PARAMS
    n = scr.WIDE_N
    want_sizes, want_shared = scr.expected("wide", k, scale)
    want = sgc.wide_expected()
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in list(scr.wide()) + [sgc.wide_query()]]
        assert (e.screen_search_index(ids[:2000], kmer=k, scale=scale) == want_sizes[:2000]).all()
        assert (e.screen_search_index_add(ids[2000:n - 10]) == want_sizes[2000:n - 10]).all()
        add = e.screen_search_add_last()
        assert add["entries"] == int(want_sizes[2000:n - 10].sum()) and add["matched_kmers"] >= 9      # motif 1: nine k-mers every genome holds
        assert (e.screen_search_count(ids[n - 10:n]) == want_sizes[n - 10:]).all()
        _rect_equals(e, want_shared[n - 10:, :n - 10], "wide, 2000 + 990")
        assert e.screen_search_last()["entries"] == int(want_sizes[:n - 10].sum())
        # all 3000 as 1500 + 1500, then the gather over the grown index
        e.screen_search_index(ids[:1500], kmer=k, scale=scale)
        e.screen_search_index_add(ids[1500:n])
        assert e.screen_search_last()["entries"] == int(want_sizes.sum())
        e.screen_gather_count(ids[n:])
        _rect_equals(e, want.hits, "wide, the gather's rectangle")
        rows = e.screen_gather_rows(np.ones(1, dtype=np.uint32))
        sgc.same_rows(rows, want, "wide, 1500 + 1500")
        assert np.array_equal(e.screen_gather_fetch(), want.left) and np.array_equal(e.screen_gather_matched(), want.matched)
        last = e.screen_gather_last()
        assert (last["claimed"], last["decrements"], last["rounds"]) == (want.claimed, want.decrements, want.rounds)


def test_mixture_over_a_grown_index():
    from pyani_amd.engine import Engine
    k, scale, need = 16, 16, 10
    want = sgc.mixture_expected(k, scale, need)
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in list(scr.family()) + list(sgc.mixture_queries())]
        e.screen_search_index(ids[:4], kmer=k, scale=scale)
        e.screen_search_index_add(ids[4:8])
        e.screen_gather_count(ids[8:])
        _rect_equals(e, want.hits, "mixture")
        sgc.same_rows(e.screen_gather_rows(np.full(3, need, dtype=np.uint32)), want, "mixture, 4 + 4")
        assert np.array_equal(e.screen_gather_fetch(), want.left) and np.array_equal(e.screen_gather_matched(), want.matched)
        last = e.screen_gather_last()
        assert (last["claimed"], last["decrements"], last["rounds"]) == (want.claimed, want.decrements, want.rounds)


# ---- 5. across 8192 ------------------------------------------------------------------------------------------------------------------------
def test_an_add_across_8192():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    split, n = 8196, sic.BEYOND_N
    hits = sic.beyond_rows(split, n)[:, :split]
    t = sic.beyond_threshold()[0]
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        assert (e.screen_search_index(ids[:8190], kmer=k, scale=scale) == sic.beyond_sizes()[:8190]).all()
        assert (e.screen_search_index_add(ids[8190:split]) == sic.beyond_sizes()[8190:split]).all()
        assert (e.screen_search_count(ids[split:]) == sic.beyond_sizes()[split:]).all()
        _rect_equals(e, hits, "beyond")
        got = e.screen_search(ids[split:], screen.ScreenOptions(t, k, scale))
        assert (got.db_sizes == sic.beyond_sizes()[:split]).all()
        assert got.pairs() == [(3, 0), (3, 8191), (3, 8192)]      # query 8199 and the three other B holders; the other queries keep nothing
        assert (got.shared == hits[3, [0, 8191, 8192]]).all()


# ---- 6. batches through a cleared store: what the add is for ---------------------------------------------------------------------------------
def test_batches_through_a_cleared_store():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = 16, 16
    genomes = scr.family()
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    qs, ds, hits = ssx.block("family", k, scale, queries, db)
    opt = screen.ScreenOptions(0.8, k, scale, 2)
    with Engine(0) as e:
        first = [e.add_genome(*genomes[g]) for g in db[:2]]
        e.screen_search_index(first, kmer=k, scale=scale, labels=[f"g{g}" for g in db[:2]])
        e.clear_genomes()
        second = [e.add_genome(*genomes[g]) for g in db[2:]]
        assert second[0] == first[0] == 0      # the ids start again: the index knows positions
        e.screen_search_index_add(second, labels=[f"g{g}" for g in db[2:]])
        e.clear_genomes()
        assert e.genome_count() == 0
        after = e.screen_search([e.add_genome(*genomes[g]) for g in queries], opt)
        _rect_equals(e, hits, "batches")
        ssx.same((after.a, after.b, after.shared), ssx.rule_block(hits, *_needs(qs, ds, k, 0.8, 2)), "batches")
        assert (after.db_sizes == ds).all() and (after.query_sizes == qs).all() and 0 < len(after.a) < hits.size
        assert after.db_labels == [f"g{g}" for g in db]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_readable(small_engines):
    from pyani_amd import _lib
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    queries, db = ssx.EDGES_QUERIES, ssx.EDGES_DB
    qs, ds, hits = ssx.block("edges", k, scale, queries, db)
    q_ids, db_ids = [ids[g] for g in queries], [ids[g] for g in db]
    need_q, need_db = np.full(4, 2, np.uint32), np.full(3, 2, np.uint32)
    want = ssx.rule_block(hits, need_q, need_db)
    zeros = dict.fromkeys(e.screen_search_add_last(), 0)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    e.screen_search_index_release()
    refused(lambda: e.screen_search_index_add([ids[4]]), "no resident search index")
    refused(lambda: e.screen_search_index_add([]), "no resident search index")
    assert e.screen_search_add_last() == zeros
    try:
        assert (e.screen_search_index(db_ids, kmer=k, scale=scale) == ds).all()
        assert (e.screen_search_count(q_ids) == qs).all()
        ssx.same(e.screen_search_select(need_q, need_db), want, "before the refusals")
        built = e.screen_search_last()

        def still_there(what):
            _rect_equals(e, hits, what)
            ssx.same(e.screen_search_select(need_q, need_db), want, what)
            now = e.screen_search_last()
            assert {x: now[x] for x in ("keys", "kmers", "entries", "slices", "index_bytes")} == {x: built[x] for x in ("keys", "kmers", "entries", "slices", "index_bytes")}
            assert e.screen_search_add_last() == zeros and e._search["n"] == 3
        refused(lambda: e.screen_search_index_add(list(range(2 ** 20 + 1 - 3))), "2^20")
        still_there("too many")
        refused(lambda: e.screen_search_index_add([ids[4], ids[2], ids[4]]), "twice")
        still_there("twice")
        refused(lambda: e.screen_search_index_add([ids[4], 10 ** 6]), "out of range")
        refused(lambda: e.screen_search_index_add([-1]), "out of range")
        still_there("out of range")
        refused(lambda: e._check(e.lib.pg_screen_search_index_add(e._h, None, 2, None)), "bad argument")
        still_there("null")
        assert len(e.screen_search_index_add([])) == 0      # nothing to add: PG_OK, and nothing changes
        e._check(e.lib.pg_screen_search_index_add(e._h, None, 0, None))
        still_there("m = 0")
        # the other resident states: an add does not touch them
        sizes70, loaded = ssc.random_symmetric(13, 70)
        e.screen_load(loaded)
        e.screen_index(db_ids, kmer=k, scale=scale)
        kept = e.screen_index_select(need_db)
        comp = e.screen_components([0, 1, 3], [1, 2, 4], None, 6)
        # an accepted add: the rectangle and the selection were n wide and go, as with a new count
        assert (e.screen_search_index_add([ids[4]]) == [ds[0]]).all()
        refused(lambda: e.screen_search_fetch(), "no counted rectangle")
        refused(lambda: e.screen_search_select(need_q, np.full(4, 2, np.uint32)), "no counted rectangle")
        refused(lambda: e._check(e.lib.pg_screen_search_read(e._h, None, None, None)), "no selection")
        refused(lambda: e.screen_gather_rows(need_q), "kept no entries")
        assert e._search["n"] == 4 and e.screen_search_add_last()["adds"] == 1 and e.screen_search_last()["query_keys"] == 0
        assert (e.screen_fetch() == loaded).all()
        ssx.same(e.screen_index_select(need_db), kept, "the index of screen_index after an add")
        for got, was in zip(e._screen_components_read(6), comp):
            assert np.array_equal(got, was)
        assert (e.screen_search_count(q_ids) == qs).all()
        _rect_equals(e, np.concatenate([hits, hits[:, :1]], axis=1), "after the add")      # genome 4 is genome 0 again
        e.screen_search_index_release()
        assert e.screen_search_add_last() == zeros      # a release zeroes the add's statistics
    finally:
        e.screen_search_index_release()
        e.screen_index_release()
        e.screen_components_release()
        e.screen_release()
