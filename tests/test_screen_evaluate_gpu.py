"""GPU: the evaluation of a partition of the kept pairs — Engine.screen_evaluate and Engine.screen_index_evaluate against
the numpy statement pyani_amd.screen.evaluate_of_pairs.  Everything is an integer and must be EQUAL, whatever the order of the list, the
length of a pair's run of duplicates, the contention on one destination, the band setting, or the path."""
import ctypes

import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_components_cases as cc
from tests import screen_evaluate_cases as ec
from tests import screen_representatives_cases as rc
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

BAND_ROWS = (1, 3, 8, 0)
NOTHING = {"n": 0, "entries": 0, "ignored": 0, "pairs": 0, "inside": 0, "clusters": 0, "select_ms": 0.0, "sort_ms": 0.0, "pair_ms": 0.0, "node_ms": 0.0}


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


def _check_last(last, a, b, label, want):
    live = int((np.asarray(a) != np.asarray(b)).sum())
    assert (last["n"], last["entries"], last["ignored"]) == (len(label), live, len(a) - live), last
    assert last["pairs"] * 2 == int(want[0][0].sum()) + int(want[0][3].sum()) and last["inside"] == int(want[1][1].sum()), last
    assert last["clusters"] == int((label == np.arange(len(label))).sum()) and last["select_ms"] == 0.0 and last["sort_ms"] > 0.0 and last["node_ms"] > 0.0, last


# ---- the list entry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,part", ec.PAIRS)
def test_list_equals_the_statement(eng, name, part):
    """Among them: star (70 000 leaves, the hub the HIGH end of every pair) under its own representatives (one cluster), its component
    and a random partition; largest (n = 2^20); heavy (2^32 - 1 weights); unweighted; the cliques (runs of 299 equal low ends)."""
    a, b, s, n, label, score = ec.case(name, part)
    want = ec.statement(name, part)
    ec.same(eng.screen_evaluate(a, b, s, n=n, label=label, score=score), want, (name, part))
    _check_last(eng.screen_evaluate_last(), a, b, label, want)
    eng.screen_evaluate_release()
    eng.screen_evaluate_release()      # nothing resident: still fine
    assert eng.screen_evaluate_last() == NOTHING


@pytest.mark.parametrize("name", sorted(ec.DIRECTED))
def test_directed_lists_equal_the_statement(eng, name):
    """Duplicate runs that end inside, at and past a wave and a workgroup's tile, the greatest weight first, last and in the middle; the
    star of 2^16 leaves in one cluster (in_weight beyond 2^32, one contended destination) and with every node its own cluster (the
    outside maxima contended), the hub the low end or the high end; the ties; the pairs of weight 0; n = 1; m = 0; unweighted; self
    entries only."""
    from pyani_amd import screen
    a, b, w, n, label, score = ec.DIRECTED[name]()
    want = screen.evaluate_of_pairs(a, b, w, n, label, score)
    got = eng.screen_evaluate(a, b, w, n=n, label=label, score=score)
    ec.same(got, want, name)
    _check_last(eng.screen_evaluate_last(), a, b, label, want)
    if name == "zero_weights":
        assert got[0][5].tolist() == [-1, 2, 1, -1] and got[0][4].tolist() == [0, 0, 0, 0] and got[1][6].tolist() == [2, -1, 0, -1]
    eng.screen_evaluate_release()


def test_list_order_direction_and_duplication_do_not_matter(eng):
    a, b, s, n, label, score = ec.case("random", "random")
    want = ec.statement("random", "random")
    order = np.random.default_rng(5).permutation(len(a))
    ec.same(eng.screen_evaluate(a[order], b[order], s[order], n=n, label=label, score=score), want, "shuffled")
    ec.same(eng.screen_evaluate(b, a, s, n=n, label=label, score=score), want, "reversed")
    ec.same(eng.screen_evaluate(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s]), n=n, label=label, score=score), want, "doubled")
    eng.screen_evaluate_release()


def test_release_and_refusals_leave_the_earlier_result(eng):
    from pyani_amd import _lib, screen
    a, b, s, n, label, score = ec.case("cliques_joined", "rep")
    want = ec.statement("cliques_joined", "rep")
    x, y = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    four = np.zeros(4, np.int32)
    lab4, score4 = np.array([0, 0, 2, 2], np.int32), np.zeros(4, np.uint64)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    def raw(x_, y_, m, n_, lab, sc):      # the library itself: the Engine's own ValueErrors come first otherwise
        ptr = lambda v: None if v is None else v.ctypes.data
        return lambda: eng._check(eng.lib.pg_screen_evaluate(eng._h, ptr(x_), ptr(y_), None, m, n_, ptr(lab), ptr(sc)))

    eng.screen_evaluate_release()
    eng.screen_evaluate_release()
    assert eng.screen_evaluate_last() == NOTHING
    refused(lambda: eng._screen_evaluate_read(n), "no resident evaluation")
    ec.same(eng.screen_evaluate(a, b, s, n=n, label=label, score=score), want, "before the refusals")
    kinds = {
        "no_node": (raw(None, None, 0, 0, lab4, score4), "nodes"),
        "too_many_nodes": (raw(None, None, 0, cc.MAX_N + 1, lab4, score4), "nodes"),
        "index_below": (raw(np.array([-1], np.int32), np.array([3], np.int32), 1, 4, lab4, score4), "outside"),
        "index_at_n": (raw(np.array([3], np.int32), np.array([4], np.int32), 1, 4, lab4, score4), "outside"),
        "null_a": (raw(None, four, 1, 4, lab4, score4), "bad argument"),
        "null_b": (raw(four, None, 1, 4, lab4, score4), "bad argument"),
        "too_many_entries": (raw(four, four, 2 ** 32, 4, lab4, score4), "entries"),
        "null_label": (raw(four, four, 1, 4, None, score4), "label"),
        "null_score": (raw(four, four, 1, 4, lab4, None), "score"),
    }
    for what, (bad, word) in ec.LABEL_REFUSALS.items():
        kinds[what] = (raw(four, four, 1, 4, np.array(bad, np.int32), score4), word)
    for what, (call, word) in kinds.items():
        refused(call, word)
        ec.same(eng._screen_evaluate_read(n), want, ("after", what))      # still readable
        assert eng.screen_evaluate_last()["n"] == n
    eng.screen_index_release()
    refused(lambda: eng.screen_index_evaluate(np.zeros(4, np.uint32), lab4, score4), "no resident index")
    # the Engine refuses as the statement does, before the library is called
    for what, (bad, word) in ec.LABEL_REFUSALS.items():
        with pytest.raises(ValueError, match=word):
            eng.screen_evaluate([0], [1], None, n=4, label=bad, score=score4)
    for call in (lambda: eng.screen_evaluate([0], [1], None, n=4, label=lab4, score=score4[:3]), lambda: eng.screen_evaluate([0], [1], None, n=4, label=None, score=score4),
                 lambda: eng.screen_evaluate([0], [4], None, n=4, label=lab4, score=score4), lambda: eng.screen_evaluate([0], [1], None, n=0, label=[], score=[]),
                 lambda: eng.screen_evaluate([0, 1], [1], None, n=4, label=lab4, score=score4)):
        with pytest.raises(ValueError):
            call()
    ec.same(eng._screen_evaluate_read(n), want, "after the refused calls")
    # any pointer of a read may be NULL
    only = np.zeros(n, np.uint64)
    eng._check(eng.lib.pg_screen_evaluate_read(eng._h, None, only.ctypes.data, None, None, None, None, None))
    assert (only == want[0][1]).all()
    only32 = np.zeros(n, np.int32)
    eng._check(eng.lib.pg_screen_evaluate_read_clusters(eng._h, None, None, None, None, only32.ctypes.data, None, None))
    assert (only32 == want[1][4]).all()
    # independent of the resident matrix, the components, the representatives and the linkage: they come and go, and so does this
    sizes, loaded = ssc.random_symmetric(13, 70)
    eng.screen_load(loaded)
    eng.screen_select(np.full(70, 3, dtype=np.uint32))
    eng.screen_release()
    comp = eng.screen_components(a, b, s, n=n)
    reps = eng.screen_representatives(a, b, s, n=n, score=score)
    link = eng.screen_linkage(a, b, np.full(len(a), 0.01), n=n, score=score)
    ec.same(eng._screen_evaluate_read(n), want, "after the other states came")
    other = ec.DIRECTED["near_tie"]()
    ec.same(eng.screen_evaluate(other[0], other[1], other[2], n=other[3], label=other[4], score=other[5]), screen.evaluate_of_pairs(*other), "a second evaluation")
    assert all((p == q).all() for p, q in zip(eng._screen_components_read(n), comp))
    assert all((p == q).all() for p, q in zip(eng._screen_representatives_read(n), reps))
    assert all((p == q).all() for p, q in zip(eng._screen_linkage_read(n), link))
    assert eng.screen_components_last()["n"] == n and eng.screen_representatives_last()["n"] == n and eng.screen_linkage_last()["n"] == n
    eng.screen_components_release()
    eng.screen_representatives_release()
    eng.screen_linkage_release()
    ec.same(eng._screen_evaluate_read(other[3]), screen.evaluate_of_pairs(*other), "after the other states went")
    eng.screen_evaluate_release()
    eng.screen_evaluate_release()
    assert eng.screen_evaluate_last() == NOTHING
    refused(lambda: eng._screen_evaluate_read(n), "no resident evaluation")


def test_multi_engine_forwards_to_the_first_engine(eng):
    from pyani_amd import multi
    a, b, s, n, label, score = ec.case("cliques", "rep")
    m = multi.MultiEngine.__new__(multi.MultiEngine)
    m.engines = [eng]
    ec.same(m.screen_evaluate(a, b, s, n=n, label=label, score=score), ec.statement("cliques", "rep"), "multi")
    assert m.screen_evaluate_last()["n"] == n
    m.screen_evaluate_release()
    assert eng.screen_evaluate_last() == NOTHING


# ---- the index entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_index_evaluation_equals_that_of_the_selected_list(small_engines, case, k, scale):
    from pyani_amd import _lib, screen
    e, ids = small_engines[case]
    n = len(ids)
    score = rc.scores("random", n)
    clusters = set()
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            for t in ssc.THRESHOLDS:
                need = screen.identity_thresholds(sizes, k, t, 2)
                a, b, s = e.screen_index_select(need)
                before = e.screen_index_last()
                for label in (screen.representatives_of_pairs(a, b, s, n, score)[0], ec.random_partition(n, 3)):
                    want = screen.evaluate_of_pairs(a, b, s, n, label, score)
                    nodes, cl, n_pairs = e.screen_index_evaluate(need, label, score)
                    assert n_pairs == len(a), (case, setting, t, n_pairs, len(a))
                    ec.same((nodes, cl), want, (case, setting, t))
                    last = e.screen_evaluate_last()
                    assert (last["n"], last["entries"], last["ignored"], last["pairs"]) == (n, len(a) // 2, 0, len(a) // 2), last      # the undirected kept pairs
                    assert last["inside"] == int(want[1][1].sum()) and last["clusters"] == int((label == np.arange(n)).sum())
                    clusters.add(last["clusters"])
                    # the index, its selection and its counters are as pg_screen_index_select left them
                    now = e.screen_index_last()
                    assert {x: now[x] for x in now if not x.endswith("_ms")} == {x: before[x] for x in before if not x.endswith("_ms")}
                    kept = [np.zeros(len(a), dt) for dt in (np.int32, np.int32, np.uint32)]
                    e._check(e.lib.pg_screen_index_read(e._h, *(x.ctypes.data if len(a) else None for x in kept)))
                    assert all((x == y).all() for x, y in zip(kept, (a, b, s)))
                    ec.same(e.screen_evaluate(a, b, s, n=n, label=label, score=score), want, (case, setting, t, "the list entry"))
                again = e.screen_index_select(need)      # a following selection is what it was
                assert all((x == y).all() for x, y in zip(again, (a, b, s)))
            # a wrong length and a missing label are refused by the library, and the result of the last call stays
            long = np.zeros(n + 1, np.int32)
            with pytest.raises(_lib.PyaniGpuError) as err:
                e.screen_index_evaluate(np.zeros(n + 1, np.uint32), long, np.zeros(n + 1, np.uint64))
            assert err.value.code == _lib.PG_E_ARG
            m = ctypes.c_uint64(0)
            with pytest.raises(_lib.PyaniGpuError) as err:
                e._check(e.lib.pg_screen_index_evaluate(e._h, need.ctypes.data, n, None, score.ctypes.data, ctypes.byref(m)))
            assert err.value.code == _lib.PG_E_ARG and "label" in str(err.value)
            ec.same(e._screen_evaluate_read(n), want, (case, setting, "after the refusals"))
        assert len(clusters) >= 2
    finally:
        e.screen_set_band(0)
        e.screen_index_release()
        e.screen_evaluate_release()


def test_evaluate_of_dense_index_and_host_are_equal(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    labels = [f"g{i}" for i in range(len(ids))]
    given = np.random.default_rng(3).random(len(ids)) * 100.0
    seen = set()
    for scores in (None, given):
        for t in (0.5, 0.8, 0.999):
            opt = screen.ScreenOptions(t, 16, 16)
            label = e.screen_dereplicate(ids, opt, scores=scores, labels=labels, path="dense").rep
            dense = e.screen_evaluate_of(ids, opt, label, scores=scores, labels=labels, path="dense")
            index = e.screen_evaluate_of(ids, opt, label, scores=scores, labels=labels, path="index")
            host = e.screen_candidates(ids, opt, labels=labels).evaluate(label, scores)      # engine=None: the statement
            for other in (index, host):
                assert other.labels == dense.labels == labels
                for f in screen.ScreenEvaluation._fields[1:]:
                    x, y = getattr(other, f), getattr(dense, f)
                    assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (t, f)
            seen.add(int((label == np.arange(len(ids))).sum()))
            assert e.screen_evaluate_last()["n"] == 0      # nothing stays resident
            with pytest.raises(Exception):
                e.screen_index_band(0)
    assert len(seen) >= 2
    with pytest.raises(ValueError):
        e.screen_evaluate_of(ids, 0.8, label, scores=given[:-1])
    with pytest.raises(ValueError):
        e.screen_evaluate_of(ids, 0.8, label[:-1])


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """The three families of the representatives' test (four genomes of 30 kb each, within a family less than 2 % apart) as FASTA files."""
    from tests import fuzz_genomes
    indir = tmp_path_factory.mktemp("evaluate") / "genomes"
    indir.mkdir()
    for stem, seq in rc.family_genomes().items():
        fuzz_genomes.write_fasta(indir / f"{stem}.fna", stem, [seq])
    return indir


def test_run_dereplicate_evaluate_and_medoid(eng, families, tmp_path):
    """evaluate=True changes nothing of what the run returned and wrote before and adds the evaluation of the clusters on the run's own
    edges; winner="medoid" makes the medoids the representatives of the same clusters."""
    from pyani_amd import screen
    from pyani_amd.subcmd_dereplicate import read_evaluation_tab, run_dereplicate
    scores = rc.family_scores()
    stems = sorted(scores)
    opt = screen.ScreenOptions(0.9, 16, 16)
    eng.clear_genomes()
    plain = run_dereplicate(families, tmp_path / "plain", screen=opt, scores=scores, write_output=True, engine=eng)
    run = run_dereplicate(families, tmp_path / "evaluated", screen=opt, scores=scores, write_output=True, engine=eng, evaluate=True)
    assert plain.evaluation is None and len(plain.written) == 3
    for f in screen.ScreenClusters._fields[1:]:
        assert (getattr(plain.clusters, f) == getattr(run.clusters, f)).all(), f
    assert plain.clusters.labels == run.clusters.labels == stems and all((x == y).all() for x, y in zip(plain.edges, run.edges))
    assert [p.name for p in run.written] == ["screen_pairs.tab", "screen_representatives.tab", "screen_clusters.tab", "screen_evaluation_genomes.tab",
                                             "screen_evaluation_clusters.tab"]
    for p, q in zip(plain.written, run.written):
        assert p.name == q.name and p.read_bytes() == q.read_bytes()
    ev = run.evaluation
    score = screen.score_keys([scores[s] for s in stems])
    assert ev.labels == stems and (ev.label == run.clusters.rep).all() and (ev.score == score).all()
    ec.same((ev.node_arrays(), ev.cluster_arrays()), screen.evaluate_of_pairs(*run.edges, len(stems), run.clusters.rep, score), "the run's edges")
    assert ev.size[ev.naming()].tolist() == [rc.PER_FAMILY] * rc.FAMILIES and ev.complete().all() and (ev.out_pairs == 0).all()
    assert ev.centrality().tobytes() == (ev.in_weight.astype(np.float64) / 3.0).tobytes()
    assert read_evaluation_tab(run.written[3])["genome"].tolist() == stems and len(read_evaluation_tab(run.written[4])) == rc.FAMILIES
    assert eng.genome_count() == 0 and eng.screen_evaluate_last()["n"] == 0 and eng.screen_representatives_last()["n"] == 0
    med = run_dereplicate(families, tmp_path / "medoid", screen=opt, scores=scores, write_output=True, engine=eng, winner="medoid")
    assert med.evaluation is not None and len(med.written) == 5
    ec.same((med.evaluation.node_arrays(), med.evaluation.cluster_arrays()), (ev.node_arrays(), ev.cluster_arrays()), "winner=medoid evaluates the same")
    assert (med.clusters.rep == ev.medoid[ev.label]).all() and (med.clusters.via == ev.to_medoid).all()
    assert med.representatives() == [stems[m] for m in sorted(ev.medoid[ev.naming()].tolist())]
    assert sorted(med.clusters.size.tolist()) == sorted(run.clusters.size.tolist()) and (ev.label[med.clusters.rep] == ev.label).all()
    with pytest.raises(ValueError, match="winner"):
        run_dereplicate(families, screen=opt, engine=eng, winner="centroid")
    # the greedy rule with exact="anim": the evaluation reads the exact edges the rule ran on
    exact = run_dereplicate(families, screen=opt, scores=scores, exact="anim", engine=eng, evaluate=True)
    assert len(exact.edges[0]) == rc.FAMILIES * 6 and int(exact.edges[2].min()) >= 950_000 and exact.written == []
    ec.same((exact.evaluation.node_arrays(), exact.evaluation.cluster_arrays()), screen.evaluate_of_pairs(*exact.edges, len(stems), exact.clusters.rep, score),
            "the exact edges")
    assert int(exact.evaluation.min[exact.evaluation.naming()].min()) >= 950_000 and exact.evaluation.complete().all()


@pytest.mark.parametrize("exact", [None, "anim"])
def test_run_dereplicate_secondary_evaluates_the_named_list(eng, families, tmp_path, exact):
    """secondary="average": exact=None evaluates the screen's kept pairs with weight = shared; exact="anim" the pairs that carry a
    distance with weight = floor(min identity * 1e6), which is exact_edges with min_ani = 0."""
    from pyani_amd import screen
    from pyani_amd.subcmd_dereplicate import exact_edges, run_dereplicate
    scores = rc.family_scores()
    stems = sorted(scores)
    score = screen.score_keys([scores[s] for s in stems])
    eng.clear_genomes()
    kw = dict(screen=screen.ScreenOptions(0.9, 16, 16), scores=scores, exact=exact, write_output=True, engine=eng, secondary="average")
    plain = run_dereplicate(families, tmp_path / "plain", **kw)
    run = run_dereplicate(families, tmp_path / "evaluated", evaluate=True, **kw)
    assert plain.evaluation is None and (plain.clusters.rep == run.clusters.rep).all() and (plain.linkage.merges == run.linkage.merges).all()
    assert [p.name for p in run.written][:4] == [p.name for p in plain.written] and [p.name for p in run.written][4:] == ["screen_evaluation_genomes.tab",
                                                                                                                       "screen_evaluation_clusters.tab"]
    for p, q in zip(plain.written, run.written):
        assert p.read_bytes() == q.read_bytes()
    if exact is None:
        edges = (run.screened.a, run.screened.b, run.screened.shared)
    else:
        edges = exact_edges(run.screened.a, run.screened.b, run.records, [run.lengths[s] for s in stems], 0.0, 0.1)
        assert len(edges[0]) == len(run.edges[0]) >= rc.FAMILIES * 6 and int(edges[2].max()) <= 1_000_000
    ev = run.evaluation
    assert (ev.label == run.linkage.rep).all()
    ec.same((ev.node_arrays(), ev.cluster_arrays()), screen.evaluate_of_pairs(*edges, len(stems), run.linkage.rep, score), exact)
    assert ev.size[ev.naming()].tolist() == [rc.PER_FAMILY] * rc.FAMILIES and ev.complete().all()
    med = run_dereplicate(families, tmp_path / "medoid", winner="medoid", **kw)
    assert (med.clusters.rep == ev.medoid[ev.label]).all() and med.linkage is not None
    assert eng.genome_count() == 0 and eng.screen_evaluate_last()["n"] == 0 and eng.screen_linkage_last()["n"] == 0
