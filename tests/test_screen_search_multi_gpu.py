"""MultiEngine.screen_search_index / screen_search (pyani_amd/multi.py): the collection dealt into contiguous ranges, one per engine, every
engine counting all queries against its range, the parts merged per query row — two engines on device 0 give the hits one engine gives."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_search_cases as ssx
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu


def _same_hits(got, want, what):
    assert got.query_labels == want.query_labels and got.db_labels == want.db_labels and got.options == want.options, what
    assert (got.query_sizes == want.query_sizes).all() and (got.db_sizes == want.db_sizes).all(), what
    ssx.same((got.a, got.b, got.shared), (want.a, want.b, want.shared), what)


def test_two_engines_on_one_gpu_give_one_engines_hits_on_family():
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    from pyani_amd.screen import ScreenOptions
    genomes = scr.family()
    queries, db = ssx.FAMILY_QUERIES, ssx.FAMILY_DB
    ql, dl = [f"g{g}" for g in queries], [f"g{g}" for g in db]
    options = [ScreenOptions(t, 16, 16, 2) for t in ssc.THRESHOLDS]
    with Engine(0) as one:
        ids = [one.add_genome(s, o) for s, o in genomes]
        one.screen_search_index([ids[g] for g in db], 16, 16, labels=dl)
        want = [one.screen_search([ids[g] for g in queries], o, query_labels=ql) for o in options]
    with MultiEngine([0, 0]) as two:
        ids = [two.add_genome(s, o) for s, o in genomes]
        sizes = two.screen_search_index([ids[g] for g in db], 16, 16, labels=dl)      # ranges [0, 2) and [2, 5)
        assert (sizes == want[0].db_sizes).all() and [e._search["n"] for e in two.engines] == [2, 3]
        two.screen_set_band(3)      # two chunks of queries on every engine
        got = [two.screen_search([ids[g] for g in queries], o, query_labels=ql) for o in options]
        two.screen_search_index_release()
        with pytest.raises(ValueError, match="no search index"):
            two.screen_search([ids[g] for g in queries], options[0])
    for g, w, o in zip(got, want, options):
        _same_hits(g, w, o)
    qs, ds, hits = ssx.block("family", 16, 16, queries, db)
    assert tuple(len(w.a) for w in want) == ssx.FAMILY_KEPT[(16, 16)]
    assert (want[1].b >= 2).any() and (want[1].b < 2).any()      # kept cells on both engines' ranges


def test_two_engines_on_one_gpu_give_one_engines_hits_on_wide():
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    from pyani_amd.screen import ScreenOptions
    k, scale = scr.WIDE_PARAMS
    split = scr.WIDE_N - 10
    opt = ScreenOptions(0.94, k, scale, 2)      # 13 of 33 k-mers: motif 1 alone (9) falls short, motif 1 and 3 (14) and the corner (18) pass
    with Engine(0) as one:
        ids = [one.add_genome(s, o) for s, o in scr.wide()]
        one.screen_search_index(ids[:split], k, scale)
        want = one.screen_search(ids[split:], opt)
    with MultiEngine([0, 0]) as two:
        ids = [two.add_genome(s, o) for s, o in scr.wide()]
        two.screen_search_index(ids[:split], k, scale)
        got = two.screen_search(ids[split:], opt)
    _same_hits(got, want, "wide")
    _, shared = scr.expected("wide", k, scale)
    assert (want.shared == shared[split:, :split][want.a, want.b]).all()
    assert 0 < len(want.a) < 10 * split and (want.b < split // 2).any() and (want.b >= split // 2).any()
