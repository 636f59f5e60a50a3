"""CPU: the host side of the screen's search — select_rectangle, the statement of its rule, against the all-vs-all rule
restricted to the rectangle; merge_search_parts; the arithmetic of SearchHits and the ties of best(); the driver's refusals.  No library
call and no device."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_search_cases as ssx
from tests import screen_select_cases as ssc


def _need(sizes, k, t, ms):
    from pyani_amd import screen
    return screen.identity_thresholds(sizes, k, t, ms)


@pytest.mark.parametrize("seed,n", [(3, 37), (4, 130)])
def test_select_rectangle_is_the_all_vs_all_rule_on_the_block(seed, n):
    from pyani_amd import screen
    sizes, shared = ssc.random_symmetric(seed, n)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    queries, db = sorted(perm[:n // 4].tolist()), sorted(perm[n // 4:].tolist())      # disjoint: no cell is a diagonal
    lengths = set()
    for k in ssc.KMERS:
        for t in ssc.THRESHOLDS:
            for ms in (1, 2):
                need = _need(sizes, k, t, ms)
                got = screen.select_rectangle(shared[np.ix_(queries, db)], need[queries], need[db])
                ssx.same(got, ssx.rule_block(shared[np.ix_(queries, db)], need[queries], need[db]), (k, t, ms))
                # ... which is what the all-vs-all rule keeps among those cells
                a, b, s = ssc.rule(shared, need)
                inside = np.isin(a, queries) & np.isin(b, db)
                want = (np.searchsorted(queries, a[inside]).astype(np.int32), np.searchsorted(db, b[inside]).astype(np.int32), s[inside])
                ssx.same(got, want, ("restricted", k, t, ms))
                ssx.same(got, ssx.restricted(shared, need, queries, db), ("restricted, by the helper", k, t, ms))
                lengths.add(len(got[0]))
    assert max(lengths) == len(queries) * len(db) and min(lengths) < len(queries) * len(db) // 2 and len(lengths) >= 4


def test_select_rectangle_has_no_diagonal():
    from pyani_amd import screen
    sizes, shared = ssc.random_symmetric(5, 40)
    queries, db = [1, 5, 7, 39], list(range(0, 40, 2)) + [5, 7]      # 5 and 7 on both sides (db positions 20 and 21)
    need = _need(sizes, 16, 0.9, 2)
    got = screen.select_rectangle(shared[np.ix_(queries, db)], need[queries], need[db])
    ssx.same(got, ssx.restricted(shared, need, queries, db), "overlap")
    for q, g in ((1, 5), (2, 7)):
        kept = bool(((got[0] == q) & (got[1] == db.index(g))).any())
        assert kept == bool(sizes[g] >= need[g]) and sizes[g] >= 2      # the genome with itself: hits = size
    assert any(((got[0] == q) & (got[1] == db.index(g))).any() for q, g in ((1, 5), (2, 7)))
    with pytest.raises(ValueError):
        screen.select_rectangle(shared[:3], need[:4], need)


@pytest.mark.parametrize("case,params,queries,db,kept", [
    ("family", (16, 16), ssx.FAMILY_QUERIES, ssx.FAMILY_DB, ssx.FAMILY_KEPT[(16, 16)]),
    ("family", (12, 16), ssx.FAMILY_QUERIES, ssx.FAMILY_DB, ssx.FAMILY_KEPT[(12, 16)]),
    ("edges", scr.EDGES_PARAMS, ssx.EDGES_QUERIES, ssx.EDGES_DB, ssx.EDGES_KEPT)])
def test_kept_counts_of_the_gpu_cases(case, params, queries, db, kept):
    from pyani_amd import screen
    k, scale = params
    qs, ds, hits = ssx.block(case, k, scale, queries, db)
    sizes, shared = scr.expected(case, k, scale)
    for ms in (1, 2):
        got = []
        for t in ssc.THRESHOLDS:
            need = _need(sizes, k, t, ms)
            sel = screen.select_rectangle(hits, _need(qs, k, t, ms), _need(ds, k, t, ms))
            ssx.same(sel, ssx.restricted(shared, need, queries, db), (case, t, ms))
            got.append(len(sel[0]))
        assert tuple(got) == kept


def test_merge_search_parts():
    from pyani_amd import screen
    sizes, shared = ssc.random_symmetric(6, 90)
    queries, db = list(range(0, 90, 9)), [g for g in range(90) if g % 9]
    hits = shared[np.ix_(queries, db)]
    need = _need(sizes, 12, 0.8, 2)
    whole = screen.select_rectangle(hits, need[queries], need[db])
    assert 0 < len(whole[0]) < hits.size
    for bounds in ([0, 80], [0, 40, 80], [0, 1, 1, 33, 80], [0, 27, 53, 80]):      # one part; two; an empty part; three uneven ones
        parts = [(lo, *screen.select_rectangle(hits[:, lo:hi], need[queries], need[db][lo:hi])) for lo, hi in zip(bounds[:-1], bounds[1:])]
        ssx.same(screen.merge_search_parts(parts), whole, bounds)
    empty = screen.merge_search_parts([])
    assert [len(x) for x in empty] == [0, 0, 0] and empty[2].dtype == np.uint32


def _hits(a, b, s, qs, ds, k=16, ms=2):
    from pyani_amd import screen
    return screen.SearchHits([f"q{i}" for i in range(len(qs))], [f"d{i}" for i in range(len(ds))], screen.ScreenOptions(0.5, k, 16, ms),
                             np.asarray(qs, np.uint32), np.asarray(ds, np.uint32), np.asarray(a, np.int32), np.asarray(b, np.int32), np.asarray(s, np.uint32))


def test_search_hits_arithmetic():
    h = _hits([0, 0, 1, 2, 2], [0, 2, 1, 0, 1], [50, 100, 1, 0, 7], qs=[100, 40, 0], ds=[200, 10, 100])
    assert h.pairs() == [(0, 0), (0, 2), (1, 1), (2, 0), (2, 1)]
    cq, cd = h.containment_query(), h.containment_db()
    assert np.array_equal(cq[:3], [0.5, 1.0, 1 / 40]) and np.isnan(cq[3:]).all()      # an empty query: NaN
    assert np.array_equal(cd, [50 / 200, 1.0, 1 / 10, 0.0, 7 / 10])
    ident = h.identity()
    # the larger containment ** (1 / k); below min_shared 0.0; an empty side does not count
    want = [np.power(np.float64(50) / np.float64(100), 1 / 16), 1.0, 0.0, 0.0, np.power(np.float64(7) / np.float64(10), 1 / 16)]
    assert np.array_equal(ident, want)
    assert np.array_equal(_hits([1], [1], [1], qs=[100, 40, 0], ds=[200, 10, 100], ms=1).identity(), [np.power(np.float64(1) / np.float64(10), 1 / 16)])
    f = h.frame()
    assert list(f.columns) == ["query", "db", "shared", "containment_query", "containment_db", "identity"]
    assert list(f["query"]) == ["q0", "q0", "q1", "q2", "q2"] and list(f["db"]) == ["d0", "d2", "d1", "d0", "d1"]
    assert np.array_equal(f["identity"].to_numpy(), ident) and list(f["shared"]) == [50, 100, 1, 0, 7]
    assert len(_hits([], [], [], qs=[1], ds=[1]).frame()) == 0


def test_the_identity_is_what_the_rule_thresholds():
    from pyani_amd import screen
    sizes, shared = ssc.random_symmetric(8, 60)
    queries, db = list(range(0, 20)), list(range(20, 60))
    hits = shared[np.ix_(queries, db)]
    for k, t, ms in ((16, 0.9, 2), (8, 0.5, 1), (12, 0.999, 2)):
        everything = screen.select_rectangle(hits, np.zeros(20, np.uint32), np.zeros(40, np.uint32))
        h = _hits(*everything, qs=sizes[queries], ds=sizes[db], k=k, ms=ms)
        kept = screen.select_rectangle(hits, _need(sizes[queries], k, t, ms), _need(sizes[db], k, t, ms))
        by_identity = h.identity() >= t
        ssx.same(kept, (h.a[by_identity], h.b[by_identity], h.shared[by_identity]), (k, t, ms))
        assert 0 < by_identity.sum() < len(by_identity)


def test_best_breaks_ties_by_the_smaller_db_index():
    # query 0: db 3 and db 1 tie at the top (same shared, same db size), db 0 is lower; query 2: one hit; query 1: none
    h = _hits([0, 0, 0, 0, 2], [0, 1, 3, 4, 2], [10, 80, 80, 79, 5], qs=[100, 50, 100], ds=[100, 400, 100, 400, 400])
    one = h.best()
    assert one.pairs() == [(0, 1), (2, 2)] and list(one.shared) == [80, 5]
    assert h.best(2).pairs() == [(0, 1), (0, 3), (2, 2)]
    assert h.best(3).pairs() == [(0, 1), (0, 3), (0, 4), (2, 2)]
    assert h.best(10).pairs() == [(0, 1), (0, 3), (0, 4), (0, 0), (2, 2)]      # by identity, not by index
    assert one.query_labels == h.query_labels and one.options == h.options and len(one.frame()) == 2
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            h.best(bad)
    assert _hits([], [], [], qs=[1], ds=[1]).best().pairs() == []


def test_driver_refusals_come_before_any_work(tmp_path):
    from pyani_amd.subcmd_search import run_screen_search

    class NoEngine:      # any use would raise AttributeError, not ValueError
        pass
    missing = tmp_path / "does_not_exist"
    with pytest.raises(ValueError, match="min_identity"):
        run_screen_search(missing, missing, engine=NoEngine())
    with pytest.raises(ValueError, match="output directory"):
        run_screen_search(missing, missing, min_identity=0.8, write_output=True, engine=NoEngine())
    with pytest.raises(ValueError, match="exact"):
        run_screen_search(missing, missing, min_identity=0.8, exact="anib", engine=NoEngine())
    with pytest.raises(ValueError, match="top"):
        run_screen_search(missing, missing, min_identity=0.8, top=0, engine=NoEngine())
    with pytest.raises(ValueError, match="8 ... 16"):
        run_screen_search(missing, missing, min_identity=0.8, kmer=17, engine=NoEngine())


def test_a_failed_build_forgets_the_index_it_released():
    """pg_screen_search_index releases the old index once its arguments pass: a refusal of the arguments leaves Engine's record of the
    old index, any later failure clears it, so that screen_search says at once that there is none (a stub library: no device)."""
    from pyani_amd import _lib
    from pyani_amd.engine import Engine

    class Lib:
        rc = 0

        def pg_screen_search_index(self, *args):
            return self.rc

        def pg_last_error(self, h):
            return b"stub"
    e = Engine.__new__(Engine)
    e.lib, e._h = Lib(), None
    e.screen_search_index([0, 1, 2], 16, 16)
    assert e._search["n"] == 3
    for rc, kept in ((_lib.PG_E_ARG, True), (_lib.PG_E_NOMEM, False)):
        e.lib.rc = rc
        with pytest.raises(_lib.PyaniGpuError):
            e.screen_search_index([0, 1], 16, 16)
        assert (e._search is not None and e._search["n"] == 3) == kept
    with pytest.raises(ValueError, match="no search index"):
        e.screen_search([0], 0.8)
