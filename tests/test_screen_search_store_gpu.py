"""GPU (through the C ABI): the resident search index exported, imported, kept in a file and shrunk (pg_screen_search_index_shape /
_export / _import / _remove, pg_screen_search_remove_last; pyani_amd/csrc/pgscr_store.inc).  An index that lost
genomes must be the index a fresh build over the survivors leaves, and an index that came back from a file the one that was saved: the
statements are the ones of the search and the gather (tests/screen_cases.py, screen_search_cases.py, screen_gather_cases.py) and
pyani_amd.screen.remove_from_search_index; everything is an integer and must be EQUAL.  The import's refusals are refusals by a
validator that only READS the values it is given: nothing here may fault."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import screen_index_cases as sic
from tests import screen_search_cases as ssx
from tests import screen_select_cases as ssc
from tests import screen_store_cases as stc

pytestmark = pytest.mark.gpu

ALL8 = list(range(8))
INDEX_FIELDS = ("keys", "kmers", "entries", "slices", "index_bytes")


def _rect_equals(e, want, what):
    got = e.screen_search_fetch()
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def _needs(qs, ds, k, t, ms):
    from pyani_amd import screen
    return screen.identity_thresholds(qs, k, t, ms), screen.identity_thresholds(ds, k, t, ms)


def _bytes_formula(last):
    return 12 * (last["kmers"] + 1) + 4 * (last["entries"] + 1) + 8 * (last["slices"] + 1) + 4 * scr.N_BINS


def _same_index(got, want, what):
    assert got[0][:6] == want[0][:6], (what, got[0], want[0])
    for g, w, name in zip(got[1], want[1], ("kmer", "start", "member", "slice_first", "bin_slice")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


def _refused(call, word=""):
    from pyani_amd import _lib
    with pytest.raises(_lib.PyaniGpuError) as err:
        call()
    assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)


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


# ---- 1. remove equals fresh ------------------------------------------------------------------------------------------------------------------
def _remove_equals_fresh(e, ids, case, k, scale, everyone, gone):
    from pyani_amd import screen
    sizes, shared = scr.expected(case, k, scale)
    left = [g for g in everyone if g not in gone]
    e.screen_search_index([ids[g] for g in everyone], kmer=k, scale=scale)
    built = e.screen_search_last()
    before = e.screen_search_index_export()
    assert built["slices"] <= 1
    e.screen_search_index_remove([everyone.index(g) for g in gone])
    rem = e.screen_search_remove_last()
    if not left:      # every column: the index is released, as a build of no genome leaves none
        assert e._search is None and rem == dict.fromkeys(rem, 0)
        _refused(lambda: e.screen_search_count([]), "no resident search index")
        return
    want_stmt = screen.remove_from_search_index(*before[1][:3], len(everyone), [everyone.index(g) for g in gone])
    if gone:
        assert (rem["genomes"], rem["entries"], rem["kmers"], rem["removes"]) == (len(gone), want_stmt[3], want_stmt[4], 1), rem
        assert rem["entries"] == int(sizes[gone].sum())
    else:
        assert rem == dict.fromkeys(rem, 0)      # nothing removed: nothing happened
    last = e.screen_search_last()
    assert last["keys"] == built["keys"] and last["kmers"] == len(want_stmt[0]) and last["entries"] == int(sizes[left].sum()), last
    if gone:
        assert last["index_bytes"] == _bytes_formula(last), last
    assert (e._search["sizes"] == sizes[left]).all() and e._search["n"] == len(left)
    got = e.screen_search_index_export()
    for g, w, name in zip(got[1][:3], want_stmt[:3], ("kmer", "start", "member")):
        assert np.array_equal(g, w.astype(g.dtype)), (gone, name)
    qs, hits = sizes[everyone], np.ascontiguousarray(shared[np.ix_(everyone, left)])
    assert (e.screen_search_count([ids[g] for g in everyone]) == qs).all()
    _rect_equals(e, hits, (case, k, scale, gone))
    for t in ssc.THRESHOLDS:
        need_q, need_db = _needs(qs, sizes[left], k, t, 2)
        ssx.same(e.screen_search_select(need_q, need_db), ssx.rule_block(hits, need_q, need_db), (case, gone, t))
    # the exported arrays are a fresh build's, element for element (one slice on both sides)
    e.screen_search_index([ids[g] for g in left], kmer=k, scale=scale)
    fresh, fresh_last = e.screen_search_index_export(), e.screen_search_last()
    assert {x: last[x] for x in ("kmers", "entries")} == {x: fresh_last[x] for x in ("kmers", "entries")}
    if last["kmers"]:
        assert last["slices"] == fresh_last["slices"] == 1
        _same_index(got, fresh, (case, gone))
    else:      # survivors without a k-mer: only the cut into slices differs (the directory stays; a fresh build has none)
        assert (last["slices"], fresh_last["slices"]) == (built["slices"], 0) and got[1][3].tolist() == [0] * (built["slices"] + 1)
        _same_index((got[0][:5], got[1][:3]), (fresh[0][:5], fresh[1][:3]), (case, gone))


@pytest.mark.parametrize("gone", ([], [0], [7], [3], [1, 5], ALL8[1:], ALL8), ids=str)
def test_remove_equals_fresh(small_engines, gone):
    e, ids = small_engines["family"]
    try:
        _remove_equals_fresh(e, ids, "family", 16, 16, ALL8, gone)
    finally:
        e.screen_search_index_release()


def test_remove_on_the_edges(small_engines):
    """Genomes without a k-mer, the twin of genome 0, and an index that keeps no k-mer at all."""
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    try:
        for gone in ([2, 3], [0], [4, 0], [0, 1, 4, 5]):
            _remove_equals_fresh(e, ids, "edges", k, scale, list(range(6)), gone)
    finally:
        e.screen_search_index_release()


# ---- 2. slices -------------------------------------------------------------------------------------------------------------------------------
def test_slices_stay_and_change_nothing(small_engines):
    e, ids = small_engines["family"]
    k, scale = 16, 16
    gone, left = [1, 5], [0, 2, 3, 4, 6, 7]
    qs, ds, hits = ssx.block("family", k, scale, ALL8, left)
    try:
        e.screen_search_index([ids[g] for g in left], kmer=k, scale=scale)
        fresh = stc.columns_of(e.screen_search_index_export())
        e.screen_search_index([ids[g] for g in ALL8], kmer=k, scale=scale)
        e.screen_set_budget(e.screen_search_last()["keys"] // 3)
        e.screen_search_index([ids[g] for g in ALL8], kmer=k, scale=scale)
        built = e.screen_search_last()["slices"]
        assert built >= 3
        e.screen_set_budget(0)
        e.screen_search_index_remove(gone)
        last = e.screen_search_last()
        shape, arrays = e.screen_search_index_export()
        assert last["slices"] == built == shape[5] and len(arrays[3]) == built + 1 and int(arrays[3][-1]) == shape[3] == len(fresh)
        assert last["index_bytes"] == _bytes_formula(last)
        assert stc.columns_of((shape, arrays)) == fresh
        assert (e.screen_search_count([ids[g] for g in ALL8]) == qs).all()
        _rect_equals(e, hits, "sliced")
    finally:
        e.screen_set_budget(0)
        e.screen_search_index_release()


# ---- 3. a slice that becomes empty -------------------------------------------------------------------------------------------------------------
def test_a_slice_becomes_empty(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    k, scale = 16, 16
    genomes = [0, 3, 4]
    try:
        e.screen_search_index([ids[g] for g in genomes], kmer=k, scale=scale)
        _, (kmer, start, member, _, _) = e.screen_search_index_export()      # the genomes' true k-mers, from the device
        of_entry = np.repeat(kmer, np.diff(start.astype(np.int64)))
        sets = [of_entry[member == c].astype(np.uint64) for c in range(3)]
        bins = [stc.bin_of(s, scale) for s in sets]
        middle = [(b >= stc.THIRDS[1]) & (b < stc.THIRDS[2]) for b in bins]
        columns = [sets[0][~middle[0]], np.unique(np.concatenate([s[m] for s, m in zip(sets, middle)])), sets[1][~middle[1]]]
        assert all(m.sum() >= 5 and (~m).sum() >= 5 for m in middle)      # every query holds k-mers of all three slices
        shape, arrays = stc.sliced_index(columns, k, scale, stc.THIRDS)
        assert screen.check_search_index(shape, *arrays) == []
        sizes = e.screen_search_index_import(shape, arrays)
        assert (sizes == [len(c) for c in columns]).all()
        want = np.array([[len(np.intersect1d(s, c)) for c in columns] for s in sets], dtype=np.uint32)
        e.screen_search_count([ids[g] for g in genomes])
        _rect_equals(e, want, "three slices, imported")
        e.screen_search_index_remove([1])
        got_shape, got = e.screen_search_index_export()
        assert got_shape[5] == 3 and got[3][1] == got[3][2] and 0 < got[3][1] < got[3][3] == got_shape[3]      # the middle slice is empty
        rem = e.screen_search_remove_last()
        assert (rem["entries"], rem["kmers"]) == (len(columns[1]), len(columns[1]))
        assert stc.columns_of((got_shape, got)) == stc.columns_of(stc.sliced_index([columns[0], columns[2]], k, scale, stc.THIRDS))
        e.screen_search_count([ids[g] for g in genomes])
        _rect_equals(e, np.ascontiguousarray(want[:, [0, 2]]), "the middle slice is empty")
        # and an add finds the empty slice: genome 3's middle k-mers come back into it
        e.screen_search_index_add([ids[3]])
        e.screen_search_count([ids[g] for g in genomes])
        back = np.array([[len(np.intersect1d(s, sets[1]))] for s in sets], dtype=np.uint32)
        _rect_equals(e, np.concatenate([want[:, [0, 2]], back], axis=1), "an add into the empty slice")
    finally:
        e.screen_search_index_release()


# ---- 4. big groups, and the 8192 edge ------------------------------------------------------------------------------------------------------------
def test_wide_groups_shrink():
    from pyani_amd.engine import Engine
    k, scale = scr.WIDE_PARAMS
    n = scr.WIDE_N
    want_sizes, want_shared = scr.expected("wide", k, scale)
    gone = list(range(0, n - 10, 2))[:1000]
    left = sorted(set(range(n - 10)) - set(gone))
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in scr.wide()]
        e.screen_search_index(ids[:n - 10], kmer=k, scale=scale)
        e.screen_search_index_remove(gone)
        rem = e.screen_search_remove_last()
        assert len(gone) == 1000 and rem["genomes"] == 1000 and rem["entries"] == int(want_sizes[gone].sum())
        assert e.screen_search_last()["entries"] == int(want_sizes[left].sum())
        assert (e.screen_search_count(ids[n - 10:n]) == want_sizes[n - 10:]).all()
        _rect_equals(e, np.ascontiguousarray(want_shared[n - 10:][:, left]), "wide, 2990 - 1000")


def test_a_remove_across_8192():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    split, n = 8196, sic.BEYOND_N
    gone = [1, 4096, 8190, 8193, 8195]
    left = [g for g in range(split) if g not in gone]
    hits = sic.beyond_rows(split, n)[:, left]
    t = sic.beyond_threshold()[0]
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        e.screen_search_index(ids[:split], kmer=k, scale=scale)
        e.screen_search_index_remove(gone)
        assert (e._search["sizes"] == sic.beyond_sizes()[left]).all() and e._search["n"] == split - 5
        assert (e.screen_search_count(ids[split:]) == sic.beyond_sizes()[split:]).all()
        _rect_equals(e, np.ascontiguousarray(hits), "beyond")
        got = e.screen_search(ids[split:], screen.ScreenOptions(t, k, scale))
        assert got.pairs() == [(3, 0), (3, left.index(8191)), (3, left.index(8192))]      # the B holders moved down with the columns
        assert (got.shared == hits[3, [0, left.index(8191), left.index(8192)]]).all()


# ---- 5. the order of operations ----------------------------------------------------------------------------------------------------------------
def test_the_order_of_operations(small_engines):
    e, ids = small_engines["family"]
    k, scale = 16, 16
    order = [0, 2, 3, 4, 6, 7, 1, 5]
    qs, ds, hits = ssx.block("family", k, scale, ALL8, order)
    try:
        e.screen_search_index([ids[g] for g in order], kmer=k, scale=scale)
        fresh, fresh_last = e.screen_search_index_export(), e.screen_search_last()
        e.screen_search_index([ids[g] for g in ALL8[:4]], kmer=k, scale=scale)
        e.screen_search_index_add([ids[g] for g in ALL8[4:]])
        e.screen_search_index_remove([1, 5])
        assert e.screen_search_add_last()["adds"] == 1 and e.screen_search_remove_last()["removes"] == 1
        e.screen_search_index_add([ids[1], ids[5]])
        _same_index(e.screen_search_index_export(), fresh, "index, add, remove, add")
        last = e.screen_search_last()
        assert {x: last[x] for x in ("kmers", "entries", "slices")} == {x: fresh_last[x] for x in ("kmers", "entries", "slices")}
        assert (e._search["sizes"] == ds).all()
        assert (e.screen_search_count([ids[g] for g in ALL8]) == qs).all()
        _rect_equals(e, hits, "index, add, remove, add")
        e.screen_search_index_remove([0])
        e.screen_search_index_remove([0])
        assert e.screen_search_remove_last()["removes"] == 3 and e._search["n"] == 6
    finally:
        e.screen_search_index_release()


def test_a_gather_after_a_remove():
    from pyani_amd.engine import Engine
    k, scale, need = 16, 16, 10
    left = [0, 1, 2, 4, 5, 7]      # genome 3, a member of the mixture, is gone: its relatives explain what they can
    fam = scr.family()
    want = sgc.gather_genomes(sgc.mixture_queries(), [fam[g] for g in left], k, scale, need)
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in list(fam) + list(sgc.mixture_queries())]
        e.screen_search_index(ids[:8], kmer=k, scale=scale)
        e.screen_search_index_remove([3, 6])
        e.screen_gather_count(ids[8:])
        _rect_equals(e, want.hits, "mixture")
        sgc.same_rows(e.screen_gather_rows(np.full(3, need, dtype=np.uint32)), want, "mixture, 8 - 2")
        assert np.array_equal(e.screen_gather_fetch(), want.left) and np.array_equal(e.screen_gather_matched(), want.matched)


# ---- 6. the round trip -------------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_a_file(tmp_path):
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale, need = 16, 16, 10
    fam, queries = scr.family(), sgc.mixture_queries()
    sizes, shared = scr.expected("family", k, scale)
    want = sgc.mixture_expected(k, scale, need)
    labels = [f"fam {g}" for g in range(8)]
    lengths = [int(o[-1]) for _, o in fam]
    path = tmp_path / "family.idx"
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in fam]
        e.screen_set_budget(10_000)      # several slices: the directory travels too
        e.screen_search_index(ids, kmer=k, scale=scale, labels=labels)
        e.screen_set_budget(0)
        saved, saved_last = e.screen_search_index_export(), e.screen_search_last()
        assert saved_last["slices"] >= 3
        e.screen_search_count(ids)
        file_bytes = e.screen_search_index_save(path, lengths=lengths)
        _rect_equals(e, shared, "a save changes nothing")
        assert path.stat().st_size == file_bytes
        e.screen_search_index_release()
        e.clear_genomes()
        q_ids = [e.add_genome(s, o) for s, o in queries]
        got_sizes, got_labels, got_lengths = e.screen_search_index_load(path)
        assert (got_sizes == sizes).all() and got_sizes.dtype == np.uint32 and got_labels == labels and got_lengths.tolist() == lengths
        assert e._search["labels"] == labels and (e._search["kmer"], e._search["scale"], e._search["n"]) == (k, scale, 8)
        _same_index(e.screen_search_index_export(), saved, "loaded")
        last = e.screen_search_last()
        assert {x: last[x] for x in ("keys", "kmers", "entries", "slices")} == {x: saved_last[x] for x in ("keys", "kmers", "entries", "slices")}
        assert last["index_bytes"] == _bytes_formula(last) and last["index_scan_ms"] == 0.0
        rem = e.screen_search_remove_last()
        assert rem == dict.fromkeys(rem, 0) and e.screen_search_add_last()["adds"] == 0
        e.screen_gather_count(q_ids)
        _rect_equals(e, want.hits, "loaded")
        qs = e.screen_search_count(q_ids)
        for t in ssc.THRESHOLDS:
            need_q, need_db = _needs(qs, sizes, k, t, 2)
            ssx.same(e.screen_search_select(need_q, need_db), ssx.rule_block(want.hits, need_q, need_db), ("loaded", t))
        e.screen_gather_count(q_ids)
        sgc.same_rows(e.screen_gather_rows(np.full(3, need, dtype=np.uint32)), want, "loaded")
        assert np.array_equal(e.screen_gather_fetch(), want.left) and np.array_equal(e.screen_gather_matched(), want.matched)
        res = e.screen_search(q_ids, screen.ScreenOptions(0.8, k, scale))
        assert res.db_labels == labels and (res.db_sizes == sizes).all()
        # an add after a load is the fresh build over the longer list
        e.screen_search_index_add([q_ids[1]], labels=["one more"])
        e.screen_search_count(q_ids)
        _rect_equals(e, np.concatenate([want.hits, want.hits[:, [1]]], axis=1), "an add after a load")      # query 1 is family genome 1
        assert e._search["labels"] == labels + ["one more"]
    with Engine(0) as other:      # a second engine loads the same file
        other.screen_search_index_load(path)
        _same_index(other.screen_search_index_export(), saved, "a second engine")
        q_ids = [other.add_genome(s, o) for s, o in queries]
        other.screen_search_count(q_ids)
        _rect_equals(other, want.hits, "a second engine")
        # stored sizes that are not the index's: a ValueError, and no index stays
        f = screen.read_search_index(path)
        wrong = tmp_path / "wrong.idx"
        screen.write_search_index(wrong, f.shape, f.arrays, f.sizes + np.uint32(1), f.labels, f.lengths)
        with pytest.raises(ValueError, match="stored sizes"):
            other.screen_search_index_load(wrong)
        assert other._search is None
        _refused(lambda: other.screen_search_count(q_ids), "no resident search index")


# ---- 7. the import's refusals ------------------------------------------------------------------------------------------------------------------
def test_import_refusals_leave_the_resident_index(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    k, scale = 16, 16
    qs, ds, hits = ssx.block("family", k, scale, ALL8, ALL8[:5])
    need_q, need_db = _needs(qs, ds, k, 0.8, 2)
    want = ssx.rule_block(hits, need_q, need_db)
    device_kinds = {"start0", "start_end", "start_order", "kmer_range", "kmer_sampled", "kmer_slice", "kmer_order", "member_range", "member_order"}
    try:
        e.screen_search_index([ids[g] for g in ALL8[:5]], kmer=k, scale=scale, labels=list("abcde"))
        e.screen_search_count([ids[g] for g in ALL8])
        built = e.screen_search_last()

        def still_there(what):
            _rect_equals(e, hits, what)
            ssx.same(e.screen_search_select(need_q, need_db), want, what)
            now = e.screen_search_last()
            assert {x: now[x] for x in INDEX_FIELDS} == {x: built[x] for x in INDEX_FIELDS}, what
            assert e._search["labels"] == list("abcde") and e._search["n"] == 5
        seen = set()
        for name, (shape, arrays, invariant) in stc.corruptions().items():
            text = screen.SEARCH_INDEX_INVARIANTS[invariant] if invariant in device_kinds else ""
            _refused(lambda: e.screen_search_index_import(shape, arrays), text)
            still_there(name)
            seen.add(invariant)
        assert device_kinds <= seen
        good_shape, good = stc.three_slices()
        _refused(lambda: e.screen_search_index_import((2 ** 20 + 1,) + good_shape[1:], good), "2^20")
        _refused(lambda: e.screen_search_index_import((0,) + good_shape[1:], good), "no genome")
        _refused(lambda: e._check(e.lib.pg_screen_search_index_import(e._h, None, None, None, None, None, None, None)), "bad argument")
        still_there("the host's refusals")
        # two corruptions at once: the first violated invariant is named, with its count
        shape, arrays, _ = stc.corruptions()["duplicate holder"]
        both = [a.copy() for a in arrays]
        both[0][[1, 5]] = both[0][[0, 4]]
        _refused(lambda: e.screen_search_index_import(shape, both), screen.SEARCH_INDEX_INVARIANTS["kmer_order"] + " (2 of them)")
        still_there("two at once")
        # an export and a shape change nothing either
        e.screen_search_index_export()
        still_there("an export")
        # the sound index is accepted, and then it is the resident one
        sizes = e.screen_search_index_import(good_shape, good)
        assert (sizes == screen.search_index_sizes(good[2], good_shape[0])).all() and e._search["n"] == 3 and e._search["kmer"] == 12
        _same_index(e.screen_search_index_export(), (good_shape, good), "the sound index")
        _refused(lambda: e.screen_search_fetch(), "no counted rectangle")
        assert e.screen_search_last()["keys"] == good_shape[6]
        # n = 0: no index is left
        empty = ((0, 16, 16, 0, 0, 0, 0), (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64), good[4]))
        assert len(e.screen_search_index_import(*empty)) == 0 and e._search is None
        _refused(lambda: e.screen_search_index_export(), "no resident search index")
    finally:
        e.screen_search_index_release()


# ---- 8. the remove's refusals --------------------------------------------------------------------------------------------------------------------
def test_remove_refusals_leave_everything_readable(small_engines):
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    queries, db = ssx.EDGES_QUERIES, ssx.EDGES_DB
    qs, ds, hits = ssx.block("edges", k, scale, queries, db)
    need_q, need_db = np.full(4, 2, np.uint32), np.full(3, 2, np.uint32)
    want = ssx.rule_block(hits, need_q, need_db)
    zeros = dict.fromkeys(e.screen_search_remove_last(), 0)
    e.screen_search_index_release()
    _refused(lambda: e.screen_search_index_remove([0]), "no resident search index")
    _refused(lambda: e.screen_search_index_remove([]), "no resident search index")
    _refused(lambda: e.screen_search_index_shape(), "no resident search index")
    try:
        e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale)
        e.screen_search_count([ids[g] for g in queries])
        built = e.screen_search_last()

        def still_there(what):
            _rect_equals(e, hits, what)
            ssx.same(e.screen_search_select(need_q, need_db), want, what)
            now = e.screen_search_last()
            assert {x: now[x] for x in INDEX_FIELDS} == {x: built[x] for x in INDEX_FIELDS}
            assert e.screen_search_remove_last() == zeros and e._search["n"] == 3
        _refused(lambda: e.screen_search_index_remove([3]), "is not in a search index of 3")
        still_there("a column >= n")
        _refused(lambda: e.screen_search_index_remove([0, 2, 0]), "twice")
        still_there("twice")
        _refused(lambda: e.screen_search_index_remove([0, 1, 2, 1]), "")
        _refused(lambda: e._check(e.lib.pg_screen_search_index_remove(e._h, None, 2)), "bad argument")
        still_there("null")
        e.screen_search_index_remove([])      # nothing to remove: PG_OK, and nothing changes
        e._check(e.lib.pg_screen_search_index_remove(e._h, None, 0))
        still_there("m = 0")
        # an accepted remove: the rectangle and the selection were n wide and go, as with a new count
        e.screen_search_index_remove([1])
        _refused(lambda: e.screen_search_fetch(), "no counted rectangle")
        _refused(lambda: e.screen_gather_rows(need_q), "kept no entries")
        assert e.screen_search_remove_last()["removes"] == 1 and e.screen_search_last()["query_keys"] == 0 and e.screen_search_last()["keys"] == built["keys"]
        e.screen_search_count([ids[g] for g in queries])
        _rect_equals(e, np.ascontiguousarray(hits[:, [0, 2]]), "after the remove")
        e.screen_search_index_release()
        assert e.screen_search_remove_last() == zeros      # a release zeroes the remove's statistics
    finally:
        e.screen_search_index_release()


# ---- 9. the drivers ----------------------------------------------------------------------------------------------------------------------------
def test_drivers(tmp_path):
    import shutil
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_gather import run_screen_gather
    from pyani_amd.subcmd_search import run_screen_search
    from pyani_amd.subcmd_searchdb import run_screen_index_build, run_screen_index_update
    k, scale = 16, 16
    fam = scr.family()
    db, qd, extra, edited = (tmp_path / x for x in ("db", "queries", "extra", "edited"))
    for d in (db, qd, extra, edited):
        d.mkdir()
    for g in range(6):
        synth.write_fasta(db / f"fam{g}.fna", *fam[g], f"fam{g}")
    for g in (6, 7):
        synth.write_fasta(extra / f"fam{g}.fna", *fam[g], f"fam{g}")
    for name, (seq, off) in zip(("mix", "copy"), sgc.mixture_queries()):
        synth.write_fasta(qd / f"{name}.fna", seq, off, name)
    index = tmp_path / "family.idx"

    def tables(run):
        return [p.read_bytes() for p in run.written]

    with Engine(0) as eng:
        built = run_screen_index_build(db, index, kmer=k, scale=scale, engine=eng)
        assert built.labels == [f"fam{g}" for g in range(6)] and eng.genome_count() == 0 and eng._search is None
        assert [built.lengths[x] for x in built.labels] == [int(fam[g][1][-1]) for g in range(6)] and index.stat().st_size == built.file_bytes
        batched = run_screen_index_build(db, tmp_path / "batched.idx", kmer=k, scale=scale, db_batch=4, engine=eng)
        assert (batched.sizes == built.sizes).all() and batched.labels == built.labels
        for run, args in ((run_screen_search, {"min_identity": 0.8}), (run_screen_gather, {"min_unique": 10})):
            a = run(db, qd, tmp_path / "from_dir", kmer=k, scale=scale, write_output=True, engine=eng, **args)
            b = run(None, qd, tmp_path / "from_index", kmer=k, scale=scale, write_output=True, engine=eng, index=index, **args)
            c = run(None, qd, tmp_path / "from_batched", kmer=k, scale=scale, write_output=True, engine=eng, index=tmp_path / "batched.idx", **args)
            assert len(tables(a)) == 2 and tables(a) == tables(b) == tables(c), run.__name__
            assert a.db_lengths == b.db_lengths and a.query_lengths == b.query_lengths
            assert eng.genome_count() == 0 and eng._search is None
            with pytest.raises(ValueError, match="was built with kmer"):
                run(None, qd, kmer=12, scale=scale, engine=eng, index=index, **args)
        # the update: fam1 and fam4 go, fam6 and fam7 join; the edited directory says the same
        updated = run_screen_index_update(index, add_dir=extra, remove=["fam4", "fam1"], out_path=tmp_path / "updated.idx", engine=eng)
        assert updated.labels == ["fam0", "fam2", "fam3", "fam5", "fam6", "fam7"] and updated.removed == ["fam4", "fam1"] and updated.added == ["fam6", "fam7"]
        assert eng.genome_count() == 0 and eng._search is None and index.stat().st_size == built.file_bytes
        for g in (0, 2, 3, 5):
            shutil.copy(db / f"fam{g}.fna", edited / f"fam{g}.fna")
        for g in (6, 7):
            shutil.copy(extra / f"fam{g}.fna", edited / f"fam{g}.fna")
        a = run_screen_search(edited, qd, tmp_path / "from_edited", min_identity=0.8, kmer=k, scale=scale, write_output=True, engine=eng)
        b = run_screen_search(None, qd, tmp_path / "from_updated", min_identity=0.8, kmer=k, scale=scale, write_output=True, engine=eng,
                              index=tmp_path / "updated.idx")
        assert tables(a) == tables(b) and len(a.hits.a) > 0
        with pytest.raises(ValueError, match="already holds a genome 'fam6'"):
            run_screen_index_update(tmp_path / "updated.idx", add_dir=extra, engine=eng)
        # in place, and a replacement: the stem leaves and comes back in one call
        again = run_screen_index_update(tmp_path / "updated.idx", add_dir=extra, remove=["fam6", "fam7"], engine=eng)
        assert again.labels == updated.labels and (again.sizes == updated.sizes).all() and again.path == tmp_path / "updated.idx"
