"""GPU (through the C ABI): the greedy representatives of the screen's kept pairs (pg_screen_representatives /
pg_screen_index_representatives / _read / _last / _release; pyani_amd/csrc/pgscr_representatives.inc) against the numpy
statement (pyani_amd.screen.representatives_of_pairs, itself held to a sequential walk by tests/test_screen_representatives_cpu.py).
Everything is an integer and must be EQUAL: whatever the order of the list, the contention on a node, the number of rounds and of
control-word batches, the band setting, or the path."""
import numpy as np
import pandas as pd
import pytest

from tests import screen_cases as scr
from tests import screen_components_cases as cc
from tests import screen_index_cases as sic
from tests import screen_representatives_cases as rc
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

BAND_ROWS = (1, 3, 8, 0)
NOTHING = {"n": 0, "entries": 0, "ignored": 0, "representatives": 0, "rounds": 0, "launches": 0, "select_ms": 0.0, "sort_ms": 0.0, "rounds_ms": 0.0, "assign_ms": 0.0}


def _same(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.uint32), ("rep", "via")):
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
@pytest.mark.parametrize("name,kind", rc.PAIRS)
def test_list_equals_the_statement(eng, name, kind):
    """Among them: star x index (the hub worst: every leaf a representative, one contended destination in the stamp, cover and assign
    passes) and star x reversed (the hub best: it covers every leaf); largest (n = 2^20); heavy (2^32 - 1 in the key's high word);
    unweighted; chain_ascending x index (2048 rounds: many control-word batches); cliques (1 round)."""
    from pyani_amd import screen
    a, b, s, n = cc.CASES[name]()
    score = rc.scores(kind, n)
    want = screen.representatives_of_pairs(a, b, s, n, score)
    got = eng.screen_representatives(a, b, s, n=n, score=score)
    _same(got, want, (name, kind))
    last = eng.screen_representatives_last()
    live = int((a != b).sum())
    assert (last["n"], last["entries"], last["ignored"]) == (n, live, len(a) - live), last
    assert last["representatives"] == int((want[0] == np.arange(n)).sum()), last
    assert 1 <= last["rounds"] <= n and last["launches"] >= last["rounds"] and last["select_ms"] == 0.0 and last["sort_ms"] > 0.0 and last["assign_ms"] > 0.0
    if (name, kind) == ("chain_ascending", "index"):
        assert last["rounds"] == 2048 and last["representatives"] == 2048, last
    if name in ("cliques", "cliques_shuffled", "one_node", "self_entries"):
        assert last["rounds"] == 1, last
    eng.screen_representatives_release()
    eng.screen_representatives_release()      # nothing resident: still fine
    assert eng.screen_representatives_last() == NOTHING


def test_list_order_direction_and_duplication_do_not_matter(eng):
    a, b, s, n = cc.CASES["random"]()
    score = rc.scores("random", n)
    want = rc.expected("random", "random")
    order = np.random.default_rng(5).permutation(len(a))
    _same(eng.screen_representatives(a[order], b[order], s[order], n=n, score=score), want, "shuffled")
    _same(eng.screen_representatives(b, a, s, n=n, score=score), want, "reversed")
    _same(eng.screen_representatives(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s]), n=n, score=score), want, "doubled")
    eng.screen_representatives_release()


def test_release_and_refusals_leave_the_earlier_result(eng):
    from pyani_amd import _lib
    a, b, s, n = cc.CASES["one_direction"]()
    score = rc.scores("reversed", n)
    want = rc.expected("one_direction", "reversed")

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    eng.screen_representatives_release()
    eng.screen_representatives_release()
    assert eng.screen_representatives_last() == NOTHING
    refused(lambda: eng._screen_representatives_read(n), "no resident representatives")
    _same(eng.screen_representatives(a, b, s, n=n, score=score), want, "before the refusals")
    for what, (bad_n, entry) in cc.REFUSALS.items():
        x, y = ([], []) if entry is None else ([entry[0]], [entry[1]])
        refused(lambda: eng.screen_representatives(x, y, None, n=bad_n, score=np.zeros(bad_n, np.uint64)), "nodes" if entry is None else "outside")
        _same(eng._screen_representatives_read(n), want, ("after", what))      # still readable
        assert eng.screen_representatives_last()["n"] == n
    refused(lambda: eng.screen_representatives(a, b, s, n=n, score=None), "score")
    refused(lambda: eng._check(eng.lib.pg_screen_representatives(eng._h, None, None, None, 1, 4, score.ctypes.data, None)), "bad argument")
    eng.screen_index_release()
    refused(lambda: eng.screen_index_representatives(np.zeros(3, np.uint32), np.zeros(3, np.uint64)), "no resident index")
    _same(eng._screen_representatives_read(n), want, "after the refused calls")
    # independent of the resident matrix and of the components: they come and go
    sizes, loaded = ssc.random_symmetric(13, 70)
    eng.screen_load(loaded)
    eng.screen_select(np.full(70, 3, dtype=np.uint32))
    eng.screen_release()
    eng.screen_components(a, b, s, n=n)
    assert eng.screen_components_last()["n"] == n and eng.screen_representatives_last()["n"] == n
    eng.screen_components_release()
    _same(eng._screen_representatives_read(n), want, "after the resident matrix and the components came and went")
    eng.screen_representatives_release()
    refused(lambda: eng._screen_representatives_read(n), "no resident representatives")


# ---- the index entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_index_representatives_equal_those_of_the_selected_list(small_engines, case, k, scale):
    from pyani_amd import _lib, screen
    e, ids = small_engines[case]
    n = len(ids)
    score = rc.scores("random", n)
    counts = set()
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            for t in ssc.THRESHOLDS:
                need = screen.identity_thresholds(sizes, k, t, 2)
                a, b, s = e.screen_index_select(need)
                before = e.screen_index_last()
                rep, via, n_pairs = e.screen_index_representatives(need, score)
                assert n_pairs == len(a), (case, setting, t, n_pairs, len(a))
                want = screen.representatives_of_pairs(a, b, s, n, score)
                _same((rep, via), want, (case, setting, t))
                last = e.screen_representatives_last()
                assert (last["n"], last["entries"], last["ignored"]) == (n, len(a) // 2, 0)      # the undirected kept pairs
                assert last["representatives"] == int((want[0] == np.arange(n)).sum())
                counts.add(last["representatives"])
                # the index, its selection and its counters are as pg_screen_index_select left them
                now = e.screen_index_last()
                assert {x: now[x] for x in now if not x.endswith("_ms")} == {x: before[x] for x in before if not x.endswith("_ms")}
                kept = [np.zeros(len(a), dt) for dt in (np.int32, np.int32, np.uint32)]
                e._check(e.lib.pg_screen_index_read(e._h, *(x.ctypes.data if len(a) else None for x in kept)))
                assert all((x == y).all() for x, y in zip(kept, (a, b, s)))
                _same(e.screen_representatives(a, b, s, n=n, score=score), want, (case, setting, t, "the list entry"))
            # a wrong length and a missing score are refused, and the result of the last call stays
            with pytest.raises(_lib.PyaniGpuError) as err:
                e.screen_index_representatives(np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64))
            assert err.value.code == _lib.PG_E_ARG
            with pytest.raises(_lib.PyaniGpuError) as err:
                e.screen_index_representatives(need, None)
            assert err.value.code == _lib.PG_E_ARG and "score" in str(err.value)
            _same(e._screen_representatives_read(n), want, (case, setting, "after the refusals"))
        assert len(counts) >= 2 and 1 in counts      # one representative at the lowest threshold, more above
    finally:
        e.screen_set_band(0)
        e.screen_index_release()
        e.screen_representatives_release()


def test_dereplicate_dense_index_and_host_are_equal(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    labels = [f"g{i}" for i in range(len(ids))]
    given = np.random.default_rng(3).random(len(ids)) * 100.0
    seen = set()
    for scores in (None, given):
        for t in (0.5, 0.8, 0.999):
            opt = screen.ScreenOptions(t, 16, 16)
            dense = e.screen_dereplicate(ids, opt, scores=scores, labels=labels, path="dense")
            index = e.screen_dereplicate(ids, opt, scores=scores, labels=labels, path="index")
            host = e.screen_candidates(ids, opt, labels=labels).representatives(scores)      # engine=None: the statement
            for other in (index, host):
                assert other.labels == dense.labels == labels
                for f in screen.ScreenClusters._fields[1:]:
                    x, y = getattr(other, f), getattr(dense, f)
                    assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (t, f)
            seen.add(len(dense.size))
            assert e.screen_representatives_last()["n"] == 0      # nothing stays resident
            with pytest.raises(Exception):
                e.screen_index_band(0)
    assert len(seen) >= 2
    with pytest.raises(ValueError):
        e.screen_dereplicate(ids, 0.8, scores=given[:-1])


def test_beyond_the_dense_limit():
    """8200 genomes, either side of the dense limit.  At the case's threshold the four holders of motif B are one cluster and the rest
    singletons; with need = 1 everywhere every pair is kept — 67 million cells, none read back — and the best-scored genome represents all."""
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = sic.BEYOND_PARAMS
    n = sic.BEYOND_N
    t, _, _ = sic.beyond_threshold()
    score = rc.scores("random", n)
    _, rank = screen.rank_order(score)
    best = int(np.flatnonzero(rank == 0)[0])
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in sic.beyond()]
        sizes = e.screen_index(ids, kmer=k, scale=scale)
        need = screen.identity_thresholds(sizes, k, t, 2)
        a, b, s = e.screen_index_select(need)
        rep, via, n_pairs = e.screen_index_representatives(need, score)
        assert n_pairs == len(a) == 12
        _same((rep, via), screen.representatives_of_pairs(a, b, s, n, score), "beyond")
        sc = screen.clusters_from_nodes(None, rep, via, score)
        holders = list(sic.BEYOND_B_HOLDERS)
        head = holders[int(np.argmin(rank[holders]))]
        assert len(sc.size) == n - 3 and sorted(np.flatnonzero(rep == head).tolist()) == holders and int(sc.size.max()) == 4
        assert e.screen_representatives_last()["representatives"] == n - 3
        rep, via, n_pairs = e.screen_index_representatives(np.ones(n, dtype=np.uint32), score)
        last = e.screen_representatives_last()
        assert n_pairs == n * (n - 1) and last["entries"] == n * (n - 1) // 2 and last["representatives"] == 1 and last["rounds"] == 1
        assert (rep == best).all() and via[best] == 0 and (np.delete(via, best) >= 1).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
def test_run_dereplicate_on_three_families(eng, tmp_path):
    """Three families of four genomes of 30 kb (tests/screen_representatives_cases.family_genomes: within a family less than 2 % apart,
    so that ANIm's identity clears min_ani = 0.95 with room — were it not to, the generator's divergence would be lowered, not the
    threshold), scores given: three representatives, each its family's best score, with exact=None and with exact="anim"."""
    from pyani_amd import screen
    from pyani_amd.subcmd_dereplicate import exact_edges, run_dereplicate
    from tests import fuzz_genomes
    indir = tmp_path / "genomes"
    indir.mkdir()
    for stem, seq in rc.family_genomes().items():
        fuzz_genomes.write_fasta(indir / f"{stem}.fna", stem, [seq])
    scores = rc.family_scores()
    stems = sorted(scores)
    best = sorted(s for s in stems if scores[s] == 100.0)
    eng.clear_genomes()
    for exact in (None, "anim"):
        out = tmp_path / f"out_{exact}"
        run = run_dereplicate(indir, out, screen=screen.ScreenOptions(0.9, 16, 16), scores=scores, exact=exact, write_output=True, engine=eng)
        assert run.clusters.labels == stems and run.representatives() == best, (exact, run.representatives())
        assert run.clusters.size.tolist() == [rc.PER_FAMILY] * rc.FAMILIES
        assert all(g[:2] == r[:2] for g, r in zip(stems, run.clusters.membership_frame()["representative"]))
        score = screen.score_keys([scores[s] for s in stems])
        assert (run.clusters.score == score).all()
        if exact is None:
            assert run.records is None
            edges = (run.screened.a, run.screened.b, run.screened.shared)
        else:
            assert len(run.records) == len(run.screened.a) and (run.records["status"] == 0).all()
            edges = exact_edges(run.screened.a, run.screened.b, run.records, [run.lengths[s] for s in stems], 0.95, 0.1)
            assert len(edges[0]) == rc.FAMILIES * 6 and int(edges[2].min()) >= 950_000      # every within-family pair is an edge
        assert all((x == y).all() for x, y in zip(edges, run.edges))
        _same((run.clusters.rep, run.clusters.via), screen.representatives_of_pairs(*edges, len(stems), score), exact)
        assert eng.genome_count() == 0 and eng.screen_representatives_last()["n"] == 0
        assert [p.name for p in run.written] == ["screen_pairs.tab", "screen_representatives.tab", "screen_clusters.tab"]
        reps = pd.read_csv(run.written[1], sep="\t", dtype={"score": np.uint64})
        members = pd.read_csv(run.written[2], sep="\t")
        pd.testing.assert_frame_equal(reps, run.clusters.frame())
        pd.testing.assert_frame_equal(members, run.clusters.membership_frame())
