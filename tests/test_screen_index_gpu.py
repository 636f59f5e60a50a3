"""GPU (through the C ABI): the screen's index path (pg_screen_index / _select / _read / _band / _last / _release, pg_screen_set_band;
pyani_amd/csrc/pg_screen.hip) against the numpy statement of the screen (tests/screen_cases.py), the numpy statement of
the selection rule (tests/screen_select_cases.rule) and the dense path.  Everything is an integer and must be EQUAL: every band the rows
of the statement's matrix, the diagonal included, every selection the same triples in the same order — whatever the band setting, the
slices, the dealing of the bands or the number of devices."""
import numpy as np
import pandas as pd
import pytest

from tests import screen_cases as scr
from tests import screen_index_cases as sic
from tests import screen_select_cases as ssc
from tests.test_run_screened_gpu import KEPT, STEMS, _options, anib_runs, anim_runs, eng, indir      # noqa: F401 — the fixtures of the screened runs

pytestmark = pytest.mark.gpu

BAND_ROWS = (1, 3, 8, 0)      # one row per band; a partial last band; one band exactly (family) or more than the rows (edges); the default
SMALL = [("family", k, s) for k, s in scr.FAMILY_PARAMS] + [("edges", *scr.EDGES_PARAMS)]


def _same(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.int32, np.uint32), "abs"):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def _band_equals(e, band, want_rows, what):
    got = e.screen_index_band(band)
    assert got.dtype == np.uint32 and got.shape == want_rows.shape, (what, band, got.shape, want_rows.shape)
    bad = np.argwhere(got != want_rows)
    assert len(bad) == 0, (what, band, len(bad), bad[:5], got[tuple(bad[0])], want_rows[tuple(bad[0])])


def _all_bands_equal(e, n, setting, shared, what):
    from pyani_amd.screen import band_ranges
    ranges = band_ranges(n, setting)
    for band, (r0, r1) in enumerate(ranges):
        _band_equals(e, band, shared[r0:r1], (what, setting))
    return len(ranges)


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


# ---- bands -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", SMALL)
def test_bands_equal_the_statement(small_engines, case, k, scale):
    e, ids = small_engines[case]
    n = len(ids)
    want_sizes, want_shared = scr.expected(case, k, scale)
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            assert sizes.dtype == np.uint32 and (sizes == want_sizes).all(), (setting, sizes, want_sizes)
            n_bands = _all_bands_equal(e, n, setting, want_shared, (case, k, scale))
            assert n_bands == {1: n, 3: -(-n // 3), 8: 1, 0: 1}[setting]
            # A full pass.  The count kernel adds one to the cell (a, b) for every grouped k-mer that a and b hold, a != b: over all bands
            #   pair_increments = sum over the k-mers held by m >= 2 genomes of m (m - 1) = sum of the off-diagonal cells
            #                   = shared.sum() - sizes.sum()        (the diagonal of `shared` is `sizes`; a k-mer of one genome adds 0)
            e.screen_index_select(np.zeros(n, dtype=np.uint32))
            last = e.screen_index_last()
            assert last["bands"] == n_bands
            assert last["pair_increments"] == int(want_shared.astype(np.int64).sum()) - int(want_sizes.astype(np.int64).sum())
            assert last["distinct"] == int(want_sizes.sum()) and last["keys"] >= last["distinct"] and last["slices"] == 1
            # E = the entries of the k-mers held by two or more genomes: sum over those k-mers of m; G of them, each with 2 <= m <= n
            assert 2 * last["groups"] <= last["entries"] <= min(n * last["groups"], last["distinct"])
            assert (last["entries"] > 0) == (last["pair_increments"] > 0)
    finally:
        e.screen_set_band(0)
        e.screen_index_release()


# ---- selection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_selection_equals_the_rule_and_the_dense_path(small_engines, case, k, scale):
    from pyani_amd import screen
    e, ids = small_engines[case]
    n = len(ids)
    want_sizes, want_shared = scr.expected(case, k, scale)
    labels = [f"g{i}" for i in range(n)]
    lengths = set()
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            for t in ssc.THRESHOLDS:
                for ms in (1, 2):
                    need = screen.identity_thresholds(sizes, k, t, ms)
                    got = e.screen_index_select(need)
                    _same(got, ssc.rule(want_shared, need), (case, setting, t, ms))
                    lengths.add(len(got[0]))
            e.screen_index_release()
            for t in ssc.THRESHOLDS:
                for ms in (1, 2):
                    opt = screen.ScreenOptions(t, k, scale, ms)
                    dense = e.screen_candidates(ids, opt, labels=labels, path="dense")
                    index = e.screen_candidates(ids, opt, labels=labels, path="index")
                    assert index.labels == dense.labels == labels and index.options == dense.options == opt
                    assert index.sizes.dtype == dense.sizes.dtype and (index.sizes == dense.sizes).all()
                    _same((index.a, index.b, index.shared), (dense.a, dense.b, dense.shared), (case, setting, t, ms))
                    with pytest.raises(Exception):      # nothing stays resident
                        e.screen_index_band(0)
        assert max(lengths) == n * (n - 1) and min(lengths) < n * (n - 1) and len(lengths) >= 3
    finally:
        e.screen_set_band(0)
        e.screen_index_release()


# ---- wide groups ---------------------------------------------------------------------------------------------------------------------------
def test_wide_groups_in_three_bands():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = scr.WIDE_PARAMS
    n = scr.WIDE_N
    want_sizes, want_shared = scr.expected("wide", k, scale)
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in scr.wide()]
        e.screen_set_band(1024)
        sizes = e.screen_index(ids, kmer=k, scale=scale)
        assert (sizes == want_sizes).all()
        assert screen.band_ranges(n, 1024) == [(0, 1024), (1024, 2048), (2048, 3000)]      # the last one of 952 rows
        _band_equals(e, 0, want_shared[0:1024], "wide")
        _band_equals(e, 2, want_shared[2048:3000], "wide")
        with pytest.raises(Exception):
            e.screen_index_band(3)
        # a threshold that only the relatives through motif 2 or motif 3 reach: halfway between the largest count of a pair that shares
        # motif 1 alone and the smallest of a pair that shares another motif too (both read off the statement)
        off = ~np.eye(n, dtype=bool)
        base = int(np.bincount(want_shared[off].astype(np.int64)).argmax())      # motif 1 alone: the bulk of the cells
        more = int(want_shared[off & (want_shared > base + 1)].min())
        cut = (base + 1 + more + 1) // 2
        assert base + 1 < cut <= more
        need = np.full(n, cut, dtype=np.uint32)
        got = e.screen_index_select(need)
        _same(got, ssc.rule(want_shared, need), "wide")
        assert 0 < len(got[0]) < n * (n - 1) and ((got[0] == 0) & (got[1] == n - 1)).any()      # the corner cell of motif 2 among them
        assert not ((got[0] == 2) & (got[1] == 6)).any()      # two genomes with motif 1 alone (2 and 6: even, no multiple of 4)
        last = e.screen_index_last()
        assert last["bands"] == 3 and last["groups"] >= 9 + 9 + 5
        assert last["pair_increments"] == int(want_shared.astype(np.int64).sum()) - int(want_sizes.astype(np.int64).sum()) > 2 ** 26


# ---- slices --------------------------------------------------------------------------------------------------------------------------------
def test_slices_do_not_change_the_index(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    n = len(ids)
    want_sizes, want_shared = scr.expected("family", 16, 16)
    need = screen.identity_thresholds(want_sizes, 16, 0.8, 2)
    try:
        e.screen_set_band(3)
        e.screen_index(ids, kmer=16, scale=16)
        one = e.screen_index_last()
        assert one["slices"] == 1
        e.screen_set_budget(one["keys"] // 3)
        sizes = e.screen_index(ids, kmer=16, scale=16)
        cut = e.screen_index_last()
        assert cut["slices"] >= 3 and (sizes == want_sizes).all()
        assert {x: cut[x] for x in ("keys", "distinct", "entries", "groups")} == {x: one[x] for x in ("keys", "distinct", "entries", "groups")}
        _all_bands_equal(e, n, 3, want_shared, "a third of the keys per slice")
        _same(e.screen_index_select(need), ssc.rule(want_shared, need), "a third of the keys per slice")
        assert 0 < len(ssc.rule(want_shared, need)[0]) < n * (n - 1)
    finally:
        e.screen_set_budget(0)
        e.screen_set_band(0)
        e.screen_index_release()


# ---- dealing -------------------------------------------------------------------------------------------------------------------------------
def test_dealt_bands_merge_into_the_single_pass(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    n = len(ids)
    want_sizes, want_shared = scr.expected("family", 16, 16)
    need = screen.identity_thresholds(want_sizes, 16, 0.5, 2)
    try:
        e.screen_set_band(1)      # eight bands
        e.screen_index(ids, kmer=16, scale=16)
        single = e.screen_index_select(need)
        _same(single, ssc.rule(want_shared, need), "single pass")
        parts, bands = [], 0
        for first in (0, 1, 2):
            parts.append(e.screen_index_select(need, band_first=first, band_step=3))
            bands += e.screen_index_last()["bands"]
            assert set(parts[-1][0].tolist()) <= set(range(first, n, 3))
        assert bands == n and all(len(p[0]) for p in parts)
        _same(screen.merge_dealt(parts), single, "dealt by three")
        assert len(e.screen_index_select(need, band_first=n, band_step=1)[0]) == 0      # no such band: nothing to work
    finally:
        e.screen_set_band(0)
        e.screen_index_release()


def test_multi_engine_on_one_device_twice_equals_one_engine(small_engines):
    from pyani_amd import screen
    from pyani_amd.multi import MultiEngine
    e, ids = small_engines["family"]
    genomes = scr.family()
    opt = screen.ScreenOptions(0.8, 16, 16)
    one = e.screen_candidates(ids, opt, path="index")
    multi = MultiEngine([0, 0])
    try:
        mids = [multi.add_genome(s, o) for s, o in genomes]
        multi.screen_set_band(3)      # three bands dealt to two engines
        got = multi.screen_candidates(mids, opt, path="index")
        dense = multi.screen_candidates(mids, opt, path="dense")
    finally:
        multi.close()
    assert 0 < len(one.a) < len(ids) * (len(ids) - 1)
    for other in (got, dense):
        assert (other.sizes == one.sizes).all() and other.options == one.options
        _same((other.a, other.b, other.shared), (one.a, one.b, one.shared), "two engines")


# ---- beyond the old limit --------------------------------------------------------------------------------------------------------------------
def test_beyond_the_dense_limit():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    n = sic.BEYOND_N
    assert n > screen.DENSE_MAX_GENOMES
    who, hand_sizes, hand_shared = sic.beyond_handful()
    t, a_only, a_and_b = sic.beyond_threshold()
    assert a_only < t < a_and_b      # the design: motif B lifts a pair clear of the rest
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        for setting, last_band, rows in ((0, 1, (8192, 8200)), (3000, 2, (6000, 8200))):
            e.screen_set_band(setting)
            assert screen.band_ranges(n, setting)[last_band] == rows and len(screen.band_ranges(n, setting)) == last_band + 1
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            assert (sizes == sic.beyond_sizes()).all()
            assert (sizes[who] == hand_sizes).all()
            band = e.screen_index_band(last_band)      # the band that holds the rows 8192 ... 8199, whole
            want = sic.beyond_rows(*rows)
            assert band.shape == want.shape
            bad = np.argwhere(band != want)
            assert len(bad) == 0, (setting, len(bad), bad[:5], band[tuple(bad[0])], want[tuple(bad[0])])
            # ... whose cells among the handful are the statement's
            in_band = [i for i, g in enumerate(who) if rows[0] <= g < rows[1]]
            assert len(in_band) >= 3
            assert (band[np.ix_([who[i] - rows[0] for i in in_band], who)] == hand_shared[in_band]).all()
            assert e.screen_index_last()["groups"] >= 9 and e.screen_index_last()["entries"] >= 9 * n      # motif A: nine groups of 8200 members
            e.screen_index_release()
            sp = e.screen_candidates(ids, screen.ScreenOptions(t, k, scale))      # "auto": the index path above 8192 genomes
            assert sp.pairs() == [(a, b) for a in sic.BEYOND_B_HOLDERS for b in sic.BEYOND_B_HOLDERS if a != b]      # 12 pairs, row-major
            pos = {g: i for i, g in enumerate(who)}
            assert (sp.shared == [hand_shared[pos[a], pos[b]] for a, b in sp.pairs()]).all() and (sp.sizes == sizes).all()
        with pytest.raises(ValueError, match="8192"):
            e.screen_candidates(ids, screen.ScreenOptions(t, k, scale), path="dense")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(small_engines):
    from pyani_amd import _lib
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    n = len(ids)
    want_sizes, want_shared = scr.expected("edges", k, scale)
    need = np.full(n, 2, dtype=np.uint32)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    e.screen_index_release()
    e.screen_index_release()      # nothing resident: still fine
    refused(lambda: e.screen_index_select(need), "no resident index")
    refused(lambda: e._check(e.lib.pg_screen_index_read(e._h, None, None, None)), "no selection")
    refused(lambda: e.screen_index_band(0), "no resident index")
    try:
        e.screen_set_band(4)
        assert (e.screen_index(ids, kmer=k, scale=scale) == want_sizes).all()
        refused(lambda: e._check(e.lib.pg_screen_index_read(e._h, None, None, None)), "no selection")      # an index, but no selection yet
        _same(e.screen_index_select(need), ssc.rule(want_shared, need), "after the refusals without an index")
        refused(lambda: e.screen_index_select(need[:n - 1]), f"not {n - 1}")
        refused(lambda: e.screen_index_select(np.zeros(n + 1, dtype=np.uint32)), f"not {n + 1}")
        refused(lambda: e.screen_index_select(need, band_step=0), "band_step")
        refused(lambda: e.screen_index([ids[0], ids[1], ids[0]], kmer=k, scale=scale), "twice")
        refused(lambda: e.screen_index(list(range(2 ** 20 + 1)), kmer=k, scale=scale), "2^20")      # (the count is checked before the ids are read)
        refused(lambda: e.screen_index(ids, kmer=17, scale=scale), "8 ... 16")
        refused(lambda: e.screen_index(ids, kmer=k, scale=3), "power of two")
        refused(lambda: e.screen_set_band(8193), "8192")
        refused(lambda: e.screen_index_band(2), "does not exist")
        # a refused screen_index leaves the earlier index in place, and a refused setting the earlier setting
        _all_bands_equal(e, n, 4, want_shared, "after refused calls")
        _same(e.screen_index_select(need), ssc.rule(want_shared, need), "after refused calls")
        # the resident matrix of screen_load and the index do not touch each other
        sizes, loaded = ssc.random_symmetric(13, 70)
        need70 = np.full(70, 3, dtype=np.uint32)
        e.screen_load(loaded)
        _all_bands_equal(e, n, 4, want_shared, "after a load")
        e.screen_index(ids, kmer=k, scale=scale)
        e.screen_index_select(need)
        e.screen_index_release()
        assert (e.screen_fetch() == loaded).all()      # survived an index build, a selection and the release
        _same(e.screen_select(need70), ssc.rule(loaded, need70), "the resident matrix after the index calls")
        e.screen_index(ids, kmer=k, scale=scale)
        e.screen_select(need70)
        e.screen_release()
        e.screen_hold(ids, kmer=k, scale=scale)
        e.screen_release()
        _all_bands_equal(e, n, 4, want_shared, "after a load, a selection, a hold and their releases")
        # the sketch mode's records are the same bytes before and after
        q, r = [ids[0], ids[1]], [ids[1], ids[0]]
        before = e.sketch_pairs(q, r, frag_len=1000, scale=16, kmer=16)
        e.screen_index(ids, kmer=k, scale=scale)
        e.screen_index_select(need)
        after = e.sketch_pairs(q, r, frag_len=1000, scale=16, kmer=16)
        assert before.tobytes() == after.tobytes()
        _all_bands_equal(e, n, 4, want_shared, "after the sketch calls")
    finally:
        e.screen_set_band(0)
    # the genome store going takes the index with it (last: the module's engine of this case has no genomes afterwards)
    e.clear_genomes()
    refused(lambda: e.screen_index_band(0), "no resident index")
    ids[:] = [e.add_genome(s, o) for s, o in scr.edges()]
    assert (e.screen_index(ids, kmer=k, scale=scale) == want_sizes).all()
    e.screen_index_release()


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------------
def _same_frames(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert list(a[name].index) == list(b[name].index) and list(a[name].columns) == list(b[name].columns)
        assert np.array_equal(a[name].to_numpy(dtype=np.float64), b[name].to_numpy(dtype=np.float64), equal_nan=True), name


def _same_screened(a, b):
    assert a.labels == b.labels and a.options == b.options and (a.sizes == b.sizes).all()
    _same((a.a, a.b, a.shared), (b.a, b.b, b.shared), "screened")


def test_run_anim_through_the_index(eng, indir, anim_runs, monkeypatch):      # noqa: F811
    from pyani_amd import screen
    from pyani_amd.subcmd_anim import run_anim
    _, _, dense, _ = anim_runs
    eng.clear_genomes()
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 4)      # six genomes: the index path
    run = run_anim(indir, skip_zero=True, engine=eng, screen=_options())
    assert [(STEMS[a], STEMS[b]) for a, b in run.screened.pairs()] == KEPT
    _same_screened(run.screened, dense.screened)
    assert run.results == dense.results and list(run.results) == list(dense.results)
    _same_frames(run.matrices, dense.matrices)      # the NaN cells included
    assert any(np.isnan(f.to_numpy(dtype=np.float64)).any() for f in run.matrices.values())
    with pytest.raises(Exception):      # the run left no index behind
        eng.screen_index_band(0)


def test_run_anib_through_the_index(eng, indir, anib_runs, monkeypatch):      # noqa: F811
    from pyani_amd import screen
    from pyani_amd.subcmd_anib import run_anib
    _, _, dense, _ = anib_runs
    eng.clear_genomes()
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 4)
    run = run_anib(indir, engine=eng, screen=_options())
    assert [(STEMS[a], STEMS[b]) for a, b in run.screened.pairs()] == KEPT
    _same_screened(run.screened, dense.screened)
    assert run.results == dense.results and list(run.results) == KEPT
    _same_frames(run.matrices, dense.matrices)
    assert all(np.isnan(f.to_numpy(dtype=np.float64)).any() for f in run.matrices.values())


def test_run_screen_through_the_index(eng, indir, tmp_path, monkeypatch):      # noqa: F811
    from pyani_amd import screen
    from pyani_amd.subcmd_screen import run_screen, tab_path
    eng.clear_genomes()
    dense = run_screen(indir, tmp_path / "dense", scale=16, min_identity=0.8, write_output=True, engine=eng)
    assert dense.result is not None and [(STEMS[a], STEMS[b]) for a, b in dense.screened.pairs()] == KEPT
    assert dense.screened.pairs() == dense.result.candidate_pairs(0.8)
    plain = run_screen(indir, scale=16, engine=eng)      # without min_identity: what it did before
    assert plain.screened is None and (plain.result.shared == dense.result.shared).all()
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 4)
    with pytest.raises(ValueError, match="min_identity"):
        run_screen(indir, scale=16, engine=eng)
    assert eng.genome_count() == 0
    run = run_screen(indir, tmp_path / "index", scale=16, min_identity=0.8, write_output=True, engine=eng)
    assert run.result is None and run.lengths == dense.lengths
    _same_screened(run.screened, dense.screened)
    assert tab_path(tmp_path / "index", "pairs").read_bytes() == tab_path(tmp_path / "dense", "pairs").read_bytes()
    tab = pd.read_csv(tab_path(tmp_path / "index", "pairs"), sep="\t")
    assert list(zip(tab["query"], tab["subject"])) == KEPT and (tab["shared"].to_numpy() == dense.screened.shared).all()
    assert not tab_path(tmp_path / "index", "shared").exists() and tab_path(tmp_path / "dense", "shared").exists()
