"""GPU (through the C ABI): the connected components of the screen's kept pairs (pg_screen_components / pg_screen_index_components / _read /
_last / _release; pyani_amd/csrc/pg_screen.hip) against the numpy statement (pyani_amd.screen.components_of_pairs, itself
held to a union-find and to scipy by tests/test_screen_components_cpu.py).  Everything is an integer and must be EQUAL: whatever the
order of the list, the contention on a cell, the upload chunks, the band setting, or the dealing of the bands."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_components_cases as cc
from tests import screen_index_cases as sic
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

BAND_ROWS = (1, 3, 8, 0)


def _same_nodes(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.uint64, np.uint64), ("root", "entries", "weight")):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


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


# ---- the list entry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_list_equals_the_statement(eng, name):
    from pyani_amd import screen
    a, b, s, n = cc.CASES[name]()
    want = screen.components_of_pairs(a, b, s, n)
    _same_nodes(want, cc.expected(name), (name, "the statement"))
    got = eng.screen_components(a, b, s, n=n)
    _same_nodes(got, want, name)
    last = eng.screen_components_last()
    live = int((a != b).sum())
    assert (last["n"], last["entries"], last["ignored"]) == (n, live, len(a) - live), last
    assert last["components"] == int((want[0] == np.arange(n)).sum()), last
    assert last["select_ms"] == 0.0 and last["hook_ms"] >= 0.0 and last["flatten_ms"] > 0.0
    if name == "random":
        assert last["components"] == cc.RANDOM_COMPONENTS
    eng.screen_components_release()
    eng.screen_components_release()      # nothing resident: still fine
    assert eng.screen_components_last() == {"n": 0, "entries": 0, "ignored": 0, "components": 0, "select_ms": 0.0, "hook_ms": 0.0, "flatten_ms": 0.0}


def test_several_upload_chunks(eng, monkeypatch):
    """A list uploaded in pieces (the development knob cuts the chunk from 2^24 entries to 65 536 and to 1000): runs of equal a are cut
    at chunk boundaries, every chunk hooks into the forest the earlier ones left."""
    for name in ("cliques_joined", "random"):
        a, b, s, n = cc.CASES[name]()
        for chunk in ("65536", "1000"):
            monkeypatch.setenv("PYANI_COMPONENTS_CHUNK", chunk)
            _same_nodes(eng.screen_components(a, b, s, n=n), cc.expected(name), (name, chunk))
    eng.screen_components_release()


def test_refusals_leave_the_earlier_result(eng):
    from pyani_amd import _lib
    a, b, s, n = cc.CASES["one_direction"]()

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    eng.screen_components_release()
    refused(lambda: eng._screen_components_read(n), "no resident components")
    _same_nodes(eng.screen_components(a, b, s, n=n), cc.expected("one_direction"), "before the refusals")
    for what, (bad_n, entry) in cc.REFUSALS.items():
        x, y = ([], []) if entry is None else ([entry[0]], [entry[1]])
        refused(lambda: eng.screen_components(x, y, None, n=bad_n), "nodes" if entry is None else "outside")
        _same_nodes(eng._screen_components_read(n), cc.expected("one_direction"), ("after", what))      # still readable
        assert eng.screen_components_last()["n"] == n
    refused(lambda: eng._check(eng.lib.pg_screen_components(eng._h, None, None, None, 1, 4, None)), "bad argument")
    refused(lambda: eng.screen_index_components(np.zeros(3, np.uint32)), "no resident index")
    _same_nodes(eng._screen_components_read(n), cc.expected("one_direction"), "after a refused index call")
    # independent of the resident matrix: a load, a selection and their release leave the components alone
    sizes, loaded = ssc.random_symmetric(13, 70)
    eng.screen_load(loaded)
    eng.screen_select(np.full(70, 3, dtype=np.uint32))
    eng.screen_release()
    _same_nodes(eng._screen_components_read(n), cc.expected("one_direction"), "after the resident matrix came and went")
    eng.screen_components_release()
    refused(lambda: eng._screen_components_read(n), "no resident components")


# ---- the index entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_index_components_equal_those_of_the_selected_list(small_engines, case, k, scale):
    from pyani_amd import screen
    e, ids = small_engines[case]
    n = len(ids)
    counts = set()
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            for t in ssc.THRESHOLDS:
                need = screen.identity_thresholds(sizes, k, t, 2)
                a, b, s = e.screen_index_select(need)
                before = e.screen_index_last()
                *got, n_pairs = e.screen_index_components(need)
                assert n_pairs == len(a), (case, setting, t, n_pairs, len(a))
                want = screen.components_of_pairs(a, b, s, n)
                _same_nodes(got, want, (case, setting, t))
                last = e.screen_components_last()
                assert (last["n"], last["entries"], last["ignored"]) == (n, len(a), 0)
                assert last["components"] == int((want[0] == np.arange(n)).sum())
                counts.add(last["components"])
                # the index, its selection and its counters are as pg_screen_index_select left them
                now = e.screen_index_last()
                assert {x: now[x] for x in now if not x.endswith("_ms")} == {x: before[x] for x in before if not x.endswith("_ms")}
                kept = [np.zeros(len(a), dt) for dt in (np.int32, np.int32, np.uint32)]
                e._check(e.lib.pg_screen_index_read(e._h, *(x.ctypes.data if len(a) else None for x in kept)))
                assert all((x == y).all() for x, y in zip(kept, (a, b, s)))
            # dealt parts merged equal the whole
            need = screen.identity_thresholds(sizes, k, 0.8, 2)
            *whole, n_whole = e.screen_index_components(need)
            parts = [e.screen_index_components(need, band_first=d, band_step=2) for d in (0, 1)]
            assert sum(p[3] for p in parts) == n_whole
            _same_nodes(screen.merge_components([p[:3] for p in parts], n, engine=e), whole, (case, setting, "dealt by two"))
            _same_nodes(screen.merge_components([p[:3] for p in parts], n), whole, (case, setting, "dealt by two, joined on the host"))
        assert len(counts) >= 2 and 1 in counts      # one component at the lowest threshold, more above
    finally:
        e.screen_set_band(0)
        e.screen_index_release()
        e.screen_components_release()


def test_components_of_dense_and_index_are_equal(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    labels = [f"g{i}" for i in range(len(ids))]
    seen = set()
    for t in (0.5, 0.8, 0.999):
        opt = screen.ScreenOptions(t, 16, 16)
        dense = e.screen_components_of(ids, opt, labels=labels, path="dense")
        index = e.screen_components_of(ids, opt, labels=labels, path="index")
        host = e.screen_candidates(ids, opt, labels=labels).components()      # engine=None: the statement
        for other in (index, host):
            assert other.labels == dense.labels == labels
            for f in screen.ScreenComponents._fields[1:]:
                x, y = getattr(other, f), getattr(dense, f)
                assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (t, f)
        seen.add(len(dense.size))
        assert e.screen_components_last()["n"] == 0      # nothing stays resident
        with pytest.raises(Exception):
            e.screen_index_band(0)
    assert len(seen) >= 2


def test_beyond_the_dense_limit():
    """8200 genomes, either side of the old limit: the index path's components against those of its own selected list, at the default
    band (two bands: 8192 + 8 rows) and at 4096 rows (three)."""
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    n = sic.BEYOND_N
    t, _, _ = sic.beyond_threshold()
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        for setting, n_bands in ((0, 2), (4096, 3)):
            e.screen_set_band(setting)
            assert len(screen.band_ranges(n, setting)) == n_bands
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            need = screen.identity_thresholds(sizes, k, t, 2)
            a, b, s = e.screen_index_select(need)
            assert list(zip(a.tolist(), b.tolist())) == [(x, y) for x in sic.BEYOND_B_HOLDERS for y in sic.BEYOND_B_HOLDERS if x != y]
            *got, n_pairs = e.screen_index_components(need)
            assert n_pairs == len(a) == 12
            _same_nodes(got, screen.components_of_pairs(a, b, s, n), ("beyond", setting))
            sc = screen.components_from_nodes(None, *got)
            assert len(sc.size) == n - 3 and sc.members(0).tolist() == list(sic.BEYOND_B_HOLDERS) and bool(sc.complete[0])
            assert e.screen_components_last()["components"] == n - 3
        # a threshold every pair reaches (motif A is in every genome): one component of 8200 through 67 million kept cells, none read back
        *got, n_pairs = e.screen_index_components(np.ones(n, dtype=np.uint32))
        assert n_pairs == n * (n - 1) and (got[0] == 0).all() and (got[1] == n - 1).all()
        assert e.screen_components_last()["components"] == 1
