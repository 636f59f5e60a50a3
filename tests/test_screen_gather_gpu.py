"""GPU (through the C ABI): the screen's gather (pg_screen_gather_count / pg_screen_gather / _read / _fetch / _matched / _last;
pyani_amd/csrc/pgscr_gather.inc) against the statement in Python sets (tests/screen_gather_cases.py).  Everything is an
integer and must be EQUAL: the rows in their order, what the rounds left of the rectangle, the matched counts and the counters —
whatever the slices of the index and of the queries, the batches of rounds or the compaction of the entries."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import screen_search_cases as ssx

pytestmark = pytest.mark.gpu

NEED = 10      # the mixture's threshold: above the handful of chance 12-mers, far below any member


def _engine(genomes):
    from pyani_amd.engine import Engine
    e = Engine(0).__enter__()
    return e, [e.add_genome(s, o) for s, o in genomes]


@pytest.fixture(scope="module")
def fam():
    """(engine, ids of the 8 family genomes, ids of the 3 mixture queries)"""
    e, ids = _engine(list(scr.family()) + list(sgc.mixture_queries()))
    yield e, ids[:8], ids[8:]
    e.__exit__(None, None, None)


def _device(e, want, need, max_ranks=65536, what=""):
    """One gather over the counted queries, held to `want`: rows, left, matched and counters; returns the rows."""
    q, n = want.hits.shape
    rows = e.screen_gather_rows(np.full(q, need, dtype=np.uint32) if np.isscalar(need) else need, max_ranks)
    sgc.same_rows(rows, want, what)
    left = e.screen_gather_fetch()
    assert left.dtype == np.uint32 and left.shape == want.left.shape and np.array_equal(left, want.left), (what, np.argwhere(left != want.left)[:5])
    matched = e.screen_gather_matched()
    assert matched.dtype == np.uint32 and np.array_equal(matched, want.matched), (what, matched, want.matched)
    last = e.screen_gather_last()
    got = {key: last[key] for key in ("entries", "rounds", "rows", "claimed", "decrements")}
    assert got == {"entries": int(want.matched.sum()), "rounds": want.rounds, "rows": len(want.query), "claimed": want.claimed, "decrements": want.decrements}, (what, got)
    sgc.check_consequences(sgc.Gathered(*rows, want.hits, left, matched, 0, 0, 0), n, max_ranks)
    return rows


# ---- mixture -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", scr.FAMILY_PARAMS)
def test_mixture(fam, k, scale):
    e, db, queries = fam
    want = sgc.mixture_expected(k, scale, NEED)
    sizes, _ = scr.expected("family", k, scale)
    try:
        assert (e.screen_search_index(db, kmer=k, scale=scale) == sizes).all()
        qsizes = e.screen_gather_count(queries)
        assert (qsizes == [len(scr.genome_set(s, o, k, scale)) for s, o in sgc.mixture_queries()]).all()
        rows = _device(e, want, NEED, what=("mixture", k, scale))
        per_query = np.bincount(rows[0], minlength=3)
        assert per_query[0] >= 2 and per_query[1] >= 1 and per_query[2] >= 1
        assert sorted(rows[1][rows[0] == 0][:2].tolist()) == [3, 7]      # the two members first, the larger overlap before the smaller
        if (k, scale) in ((16, 16), (16, 256)):
            # the decomposition is the two members and nothing else, while a search at a low threshold lists every relative of genome 3
            assert per_query.tolist() == [2, 1, 1] and rows[1].tolist() == [3, 7, 0, 5]
            a, b, s = e.screen_search_select(np.full(3, NEED, np.uint32), np.full(8, NEED, np.uint32))
            assert (a == 0).sum() > per_query[0] and (a == 0).sum() >= 7
        # another gather over the same count, every k-mer worth a row: the entries and the rectangle were left as the count made them
        _device(e, sgc.mixture_expected(k, scale, 1), 1, what=("mixture, need 1", k, scale))
    finally:
        e.screen_search_index_release()


# ---- the rectangle stays -----------------------------------------------------------------------------------------------------------------
def test_the_rectangle_stays(fam):
    from pyani_amd import screen
    e, db, queries = fam
    k, scale = 16, 16
    want = sgc.mixture_expected(k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        qsizes = e.screen_gather_count(queries)
        before = e.screen_search_fetch()
        assert np.array_equal(before, want.hits)
        _device(e, want, NEED, what="stays")
        assert np.array_equal(e.screen_search_fetch(), want.hits)
        assert e.screen_search_last()["increments"] == int(want.hits.astype(np.int64).sum())
        dsizes = scr.expected("family", k, scale)[0]
        for t in (0.8, 0.95):
            need_q, need_db = screen.identity_thresholds(qsizes, k, t, 2), screen.identity_thresholds(dsizes, k, t, 2)
            ssx.same(e.screen_search_select(need_q, need_db), ssx.rule_block(want.hits, need_q, need_db), ("select after a gather", t))
        left = e.screen_gather_fetch()
        assert np.array_equal(left, want.left) and (left[want.query, want.db] == 0).all() and (left != want.hits).any()
    finally:
        e.screen_search_index_release()


# ---- ties --------------------------------------------------------------------------------------------------------------------------------
def test_ties(fam):
    e, db, _ = fam
    k, scale = 16, 16
    sizes, _ = scr.expected("family", k, scale)
    assert sizes[0] == sizes[1] == sizes[2]      # the ancestor, its copy, its reverse complement: one canonical set
    try:
        for order in (list(range(8)), [2, 1, 0, 3, 4, 5, 6, 7]):
            fam_genomes = scr.family()
            want = sgc.gather_genomes([fam_genomes[1]], [fam_genomes[g] for g in order], k, scale, 1)
            e.screen_search_index([db[g] for g in order], kmer=k, scale=scale)
            e.screen_gather_count([db[1]])
            rows = _device(e, want, 1, what=("ties", order))
            assert rows[1].tolist() == [0] and rows[2].tolist() == [sizes[1]] and rows[3].tolist() == [sizes[1]]
            assert (e.screen_gather_fetch()[0, :3] == 0).all()
    finally:
        e.screen_search_index_release()


# ---- wide --------------------------------------------------------------------------------------------------------------------------------
def test_wide():
    k, scale = scr.WIDE_PARAMS
    e, ids = _engine(list(scr.wide()) + [sgc.wide_query()])
    want = sgc.wide_expected()
    assert list(zip(want.db.tolist(), want.unique.tolist(), want.total.tolist())) == [(0, 33, 33), (4, 24, 33)] and not want.left.any()
    assert want.decrements >= 9 * scr.WIDE_N      # the first claim walks the 9 groups that all 3000 genomes hold
    try:
        e.screen_search_index(ids[:scr.WIDE_N], kmer=k, scale=scale)
        e.screen_gather_count(ids[scr.WIDE_N:])
        _device(e, want, 1, what="wide")
    finally:
        e.__exit__(None, None, None)


# ---- many ranks --------------------------------------------------------------------------------------------------------------------------
def test_many_ranks(monkeypatch):
    k, scale = sgc.MANY_PARAMS
    e, ids = _engine(list(sgc.many()) + [sgc.join(sgc.many())])
    full = sgc.many_expected()
    assert full.db.tolist() == list(range(sgc.MANY_N - 1, -1, -1)) and full.rounds == sgc.MANY_N + 1 > 32      # the largest first; more than two batches of rounds
    try:
        sizes = e.screen_search_index(ids[:sgc.MANY_N], kmer=k, scale=scale)
        e.screen_gather_count(ids[sgc.MANY_N:])
        _device(e, full, 1, what="many")
        monkeypatch.setenv("PYANI_GATHER_COMPACT", "0")      # (a development switch: the entries never move into a shorter list)
        _device(e, full, 1, what="many, no compaction")
        monkeypatch.delenv("PYANI_GATHER_COMPACT")
        for max_ranks in (1, 7):
            want = sgc.many_expected(1, max_ranks)
            assert want.db.tolist() == full.db.tolist()[:max_ranks]
            _device(e, want, 1, max_ranks, what=("many", max_ranks))
        above = int(sizes.max()) + 1
        none = _device(e, sgc.many_expected(above), above, what="many, none")
        assert len(none[0]) == 0 and np.array_equal(e.screen_gather_fetch(), full.hits)
    finally:
        e.__exit__(None, None, None)


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
def test_edges():
    k, scale = scr.EDGES_PARAMS
    genomes = scr.edges()
    e, ids = _engine(genomes)
    db, queries = ssx.EDGES_DB, [scr.EDGES_SHORT, scr.EDGES_N_ONLY, 1]
    want = sgc.gather_genomes([genomes[g] for g in queries], [genomes[g] for g in db], k, scale, 1)
    assert want.matched[0] == want.matched[1] == 0 and (want.query == 2).all() and len(want.query) >= 1
    try:
        e.screen_search_index([ids[g] for g in db], kmer=k, scale=scale)
        assert e.screen_gather_count([ids[g] for g in queries]).tolist()[:2] == [0, 0]
        _device(e, want, 1, what="edges")
        # no query at all: no rows, nothing to fetch
        assert len(e.screen_gather_count([])) == 0
        rows = e.screen_gather_rows(np.zeros(0, np.uint32))
        assert [len(x) for x in rows] == [0, 0, 0, 0] and e.screen_gather_fetch().shape == (0, 3)
        last = e.screen_gather_last()
        assert last["rows"] == last["rounds"] == last["entries"] == 0
    finally:
        e.__exit__(None, None, None)


# ---- slices ------------------------------------------------------------------------------------------------------------------------------
def test_slices(fam):
    e, db, queries = fam
    k, scale = 16, 16
    want = sgc.mixture_expected(k, scale, NEED)
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        e.screen_gather_count(queries)
        one = e.screen_search_last()
        assert one["slices"] == one["query_slices"] == 1
        e.screen_set_budget(min(one["keys"], one["query_keys"]) // 3)
        e.screen_search_index(db, kmer=k, scale=scale)
        e.screen_gather_count(queries)
        three = e.screen_search_last()
        assert three["slices"] >= 3 and three["query_slices"] >= 3
        _device(e, want, NEED, what="slices")
    finally:
        e.screen_set_budget(0)
        e.screen_search_index_release()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(fam):
    from pyani_amd import _lib
    e, db, queries = fam
    k, scale = 16, 16
    want = sgc.mixture_expected(k, scale, NEED)
    need = np.full(3, NEED, np.uint32)

    def refused(call, message):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and message in str(err.value), str(err.value)

    def still_readable():
        import ctypes
        r = len(want.query)
        out = [np.zeros(r, np.int32), np.zeros(r, np.int32), np.zeros(r, np.uint32), np.zeros(r, np.uint32)]
        assert e.lib.pg_screen_gather_read(e._h, *(ctypes.c_void_p(x.ctypes.data) for x in out)) == 0
        sgc.same_rows(out, want, "after a refusal")
        assert np.array_equal(e.screen_gather_fetch(), want.left)

    e.screen_search_index_release()
    refused(lambda: e.screen_gather_rows(need), "no resident search index")
    try:
        e.screen_search_index(db, kmer=k, scale=scale)
        e.screen_search_count(queries)
        refused(lambda: e.screen_gather_rows(need), "kept no entries")
        refused(lambda: e.screen_gather_matched(), "kept no entries")
        e.screen_gather_count(queries)
        refused(lambda: e.screen_gather_fetch(), "no gathered rows")
        _device(e, want, NEED, what="before the refusals")
        refused(lambda: e.screen_gather_rows(need[:2]), "3 queries, not 2")
        still_readable()
        for bad in (0, 65537):
            refused(lambda: e.screen_gather_rows(need, bad), "max_ranks")
        still_readable()
        import ctypes
        r = ctypes.c_uint64(0)
        assert e.lib.pg_screen_gather(e._h, None, 3, 5, ctypes.byref(r)) == _lib.PG_E_ARG
        still_readable()
        # a plain count drops the entries and the rows
        e.screen_search_count(queries)
        refused(lambda: e.screen_gather_fetch(), "no gathered rows")
        assert e.screen_gather_last()["entries"] == 0
    finally:
        e.screen_search_index_release()


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    from pyani_amd import synth
    db, qd = tmp_path_factory.mktemp("gather_db"), tmp_path_factory.mktemp("gather_queries")
    for g, (seq, off) in enumerate(scr.family()):
        synth.write_fasta(db / f"fam{g}.fna", seq, off, f"fam{g}")
    for name, (seq, off) in zip(("mix", "copy"), sgc.mixture_queries()):
        synth.write_fasta(qd / f"{name}.fna", seq, off, name)
    return db, qd


def test_driver(dirs, tmp_path):
    import pandas as pd
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_gather import gather_tab_path, run_screen_gather
    db_dir, q_dir = dirs
    k, scale = 16, 16
    queries = sgc.mixture_queries()
    want = sgc.gather_genomes([queries[1], queries[0]], scr.family(), k, scale, NEED)      # file order: copy.fna, mix.fna
    with Engine(0) as eng:
        run = run_screen_gather(db_dir, q_dir, tmp_path, min_unique=NEED, kmer=k, scale=scale, write_output=True, engine=eng)
        assert eng.genome_count() == 0 and run.exact is None
        with pytest.raises(Exception):      # the run left no index behind
            eng.screen_search_count([])
        r = run.result
        assert r.query_labels == ["copy", "mix"] and r.db_labels == [f"fam{g}" for g in range(8)]
        sgc.same_rows((r.query, r.db, r.unique, r.total), want, "driver")
        assert np.array_equal(r.matched, want.matched)
        assert list(zip(run.frame["query"], run.frame["db"])) == [("copy", "fam0"), ("mix", "fam3"), ("mix", "fam7")]
        assert run.written == [gather_tab_path(tmp_path, "rows"), gather_tab_path(tmp_path, "summary")]
        rows_tab, summary_tab = (pd.read_csv(p, sep="\t", float_precision="round_trip") for p in run.written)
        assert list(rows_tab.columns) == ["query", "rank", "db", "unique", "total", "f_unique_query", "f_unique_cumulative", "f_match", "identity"]
        assert list(summary_tab.columns) == ["query", "size", "matched", "rows", "explained", "unexplained"]
        for tab, frame in ((rows_tab, run.frame), (summary_tab, run.summary)):
            for c in frame.columns:
                if frame[c].dtype == object:
                    assert list(tab[c]) == list(frame[c]), c
                else:
                    assert np.array_equal(tab[c].to_numpy(dtype=np.float64), frame[c].to_numpy(dtype=np.float64), equal_nan=True), c
        assert list(summary_tab["rows"]) == [1, 2] and list(summary_tab["explained"]) == [int(want.unique[0]), int(want.unique[1:].sum())]
        mix = rows_tab[rows_tab["query"] == "mix"]
        assert 0.6 < mix["f_unique_cumulative"].iloc[-1] < 0.7 and (mix["identity"] > 0.99).all()      # two thirds of the mixture are the two members
        with pytest.raises(ValueError, match="single engine"):
            run_screen_gather(db_dir, q_dir, min_unique=NEED, devices=[0], engine=eng)
        with pytest.raises(ValueError, match="min_unique"):
            run_screen_gather(db_dir, q_dir, engine=eng)
        # exact="anim": the recorded rows and nothing else
        exact = run_screen_gather(db_dir, q_dir, min_unique=NEED, kmer=k, scale=scale, exact="anim", engine=eng)
        assert eng.genome_count() == 0 and exact.written == []
        assert sorted(exact.exact) == [("fam0", "copy"), ("fam3", "mix"), ("fam7", "mix")]
        assert list(exact.frame.columns)[9:] == ["anim_identity", "anim_coverage_db"]
        for row in exact.frame.itertuples():
            assert row.anim_identity > 0.999 and 0.99 < row.anim_coverage_db <= 1.0, row
