"""CPU-only: the statement of the evaluation (pyani_amd.screen.evaluate_of_pairs) against a brute force of the tests'
own, its invariants and refusals, the ScreenEvaluation's frames, and the two tables written and read back.  Everything is an integer and
must be EQUAL; the one float, centrality(), is compared bit for bit with the same division done here."""
import numpy as np
import pandas as pd
import pytest

from tests import screen_components_cases as cc
from tests import screen_evaluate_cases as ec
from tests import screen_representatives_cases as rc


@pytest.mark.parametrize("part", ec.PARTITIONS)
@pytest.mark.parametrize("name", ec.BRUTE_CASES)
def test_statement_equals_the_brute_force(name, part):
    a, b, s, n, label, score = ec.case(name, part)
    ec.same(ec.statement(name, part), ec.brute(a, b, s, n, label, score), (name, part))


@pytest.mark.parametrize("name", sorted(ec.DIRECTED))
def test_statement_equals_the_brute_force_on_the_directed_lists(name):
    from pyani_amd import screen
    args = ec.DIRECTED[name]()
    ec.same(screen.evaluate_of_pairs(*args), ec.brute(*args), name)


def test_directed_lists_say_what_their_docstrings_say():
    from pyani_amd import screen

    def named(args):
        nodes, clusters = screen.evaluate_of_pairs(*args)
        return dict(zip(ec.NODE_ARRAYS, nodes)), dict(zip(ec.CLUSTER_ARRAYS, clusters))
    for count in ec.RUN_LENGTHS:
        for place in ec.RUN_PLACES:
            v, c = named(ec.duplicate_run(count, place))
            assert v["in_pairs"].tolist() == [0, 0, 2, 0, 0, 1, 1, 0] and v["in_weight"][2] == 9 + count + 4 and v["in_min"][2] == 4
            assert v["in_weight"][5] == 9 + count and c["pairs"][2] == 2 and c["near_weight"][2] == 3 and c["near_cluster"][2] == 0
    v, c = named(ec.star(False, False))
    assert int(v["in_weight"][0]) == ec.STAR_LEAVES * ec.TOP > 2 ** 32 and int(c["medoid"][0]) == 0 and int(c["pairs"][0]) == ec.STAR_LEAVES
    assert (v["to_medoid"][1:] == ec.TOP).all() and v["to_medoid"][0] == 0 and (v["out_pairs"] == 0).all()
    v, c = named(ec.star(True, True))
    hub = ec.STAR_LEAVES
    assert int(v["out_pairs"][hub]) == ec.STAR_LEAVES and int(v["out_node"][hub]) == 0 and int(c["near_cluster"][hub]) == 0
    assert (v["out_node"][:hub] == hub).all() and (c["size"] == 1).all() and (c["medoid"] == np.arange(hub + 1)).all()
    assert int(named(ec.medoid_tie(True))[1]["medoid"][0]) == 3 and int(named(ec.medoid_tie(False))[1]["medoid"][0]) == 4
    v, c = named(ec.near_tie())
    assert c["near_cluster"].tolist() == [2, -1, 0, -1, 0, -1] and c["near_weight"].tolist() == [7, 0, 7, 0, 7, 0] and v["out_node"].tolist() == [2, 4, 0, 0, 1, -1]
    v, c = named(ec.zero_weights())
    assert v["in_min"].tolist() == [0, 0, ec.NONE, ec.NONE] and v["in_pairs"].tolist() == [1, 1, 0, 0]
    assert v["out_node"].tolist() == [-1, 2, 1, -1] and v["out_weight"].tolist() == [0, 0, 0, 0] and v["out_pairs"].tolist() == [0, 1, 1, 0]
    assert c["near_cluster"].tolist() == [2, -1, 0, -1] and c["min"].tolist() == [0, 0, ec.NONE, ec.NONE]
    v, c = named(ec.tiny("self_only"))
    assert all((x == 0).all() for k, x in v.items() if k not in ("in_min", "out_node")) and (v["in_min"] == ec.NONE).all() and (v["out_node"] == -1).all()
    assert c["size"].tolist() == [3, 0, 0, 2, 0] and c["medoid"].tolist() == [0, -1, -1, 3, -1]


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_invariants(name):
    for part in ec.PARTITIONS:
        label = ec.case(name, part)[4]
        nodes, clusters = (dict(zip(k, x)) for k, x in zip((ec.NODE_ARRAYS, ec.CLUSTER_ARRAYS), ec.statement(name, part)))
        assert int(nodes["in_pairs"].sum()) == 2 * int(clusters["pairs"].sum()), (name, part)
        assert int(nodes["in_weight"].sum()) == 2 * int(clusters["weight"].sum())
        assert int(clusters["size"].sum()) == len(label) and (clusters["size"][label] >= 1).all()
        names = label == np.arange(len(label))
        assert (label[clusters["medoid"][names]] == np.flatnonzero(names)).all() and (clusters["medoid"][~names] == -1).all()
        if part == "root":      # no pair leaves a component
            assert (nodes["out_pairs"] == 0).all() and (nodes["out_node"] == -1).all() and (nodes["out_weight"] == 0).all()
            assert (clusters["near_cluster"] == -1).all() and (clusters["near_weight"] == 0).all()


def test_order_direction_and_duplication_do_not_matter():
    from pyani_amd import screen
    a, b, s, n, label, score = ec.case("random", "rep")
    want = ec.statement("random", "rep")
    order = np.random.default_rng(5).permutation(len(a))
    ec.same(screen.evaluate_of_pairs(a[order], b[order], s[order], n, label, score), want, "shuffled")
    ec.same(screen.evaluate_of_pairs(b, a, s, n, label, score), want, "reversed")
    ec.same(screen.evaluate_of_pairs(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s]), n, label, score), want, "doubled")


def test_refusals():
    from pyani_amd import screen
    score = np.zeros(4, np.uint64)
    for what, (bad_n, entry) in cc.REFUSALS.items():
        x, y = ([], []) if entry is None else ([entry[0]], [entry[1]])
        with pytest.raises(ValueError):
            screen.evaluate_of_pairs(x, y, None, bad_n, np.zeros(max(bad_n, 0), np.int32) if bad_n <= 8 else None, np.zeros(max(bad_n, 0) if bad_n <= 8 else 0, np.uint64))
    for what, (label, word) in ec.LABEL_REFUSALS.items():
        with pytest.raises(ValueError, match=word):
            screen.evaluate_of_pairs([0], [1], None, 4, label, score)
        with pytest.raises(ValueError, match=word):
            screen.check_partition(label, 4)
    with pytest.raises(ValueError, match="labels"):
        screen.evaluate_of_pairs([0], [1], None, 4, [0, 0, 2], score)
    with pytest.raises(ValueError, match="scores"):
        screen.evaluate_of_pairs([0], [1], None, 4, [0, 0, 2, 2], score[:3])
    with pytest.raises(ValueError, match="same length"):
        screen.evaluate_of_pairs([0, 1], [1], None, 4, [0, 0, 2, 2], score)
    with pytest.raises(ValueError, match="same length"):
        screen.evaluate_of_pairs([0], [1], [1, 2], 4, [0, 0, 2, 2], score)
    assert screen.EVALUATE_MAX_ENTRIES == 2 ** 32 - 1
    with pytest.raises(ValueError):
        screen.evaluation_from_nodes(None, [0, 0], np.zeros(2, np.uint64), [np.zeros(2)] * 6, [np.zeros(2)] * 7)
    with pytest.raises(ValueError):
        screen.evaluation_from_nodes(None, [0, 0], np.zeros(2, np.uint64), [np.zeros(3)] * 7, [np.zeros(2)] * 7)
    with pytest.raises(ValueError, match="medoid"):
        screen.evaluation_from_nodes(None, [0, 0, 2], np.zeros(3, np.uint64), [np.zeros(3)] * 7, [np.zeros(3)] * 4 + [[2, -1, 2]] + [np.zeros(3)] * 2)


def _evaluation(name, part, labels=True):
    from pyani_amd import screen
    a, b, s, n, label, score = ec.case(name, part)
    return screen.evaluation_from_nodes([f"g{v}" for v in range(n)] if labels else None, label, score, *ec.statement(name, part))


def test_frames_and_centrality():
    from pyani_amd import screen
    ev = _evaluation("cliques_joined", "root")
    n = 2 * cc.CLIQUE
    assert ev.naming().tolist() == [0] and ev.cluster_of().tolist() == [0] * n
    want = ev.in_weight.astype(np.float64) / np.float64(n - 1)
    assert ev.centrality().dtype == np.float64 and ev.centrality().tobytes() == want.tobytes()
    t = ev.cluster_frame()
    assert list(t.columns) == ["cluster", "name", "size", "pairs", "complete", "weight", "mean_weight", "min", "medoid", "near_weight", "near_cluster"]
    assert t["size"].tolist() == [n] and t["pairs"].tolist() == [cc.CLIQUE * (cc.CLIQUE - 1) + 1] and t["complete"].tolist() == [False]
    assert t["mean_weight"].tolist() == [float(ev.weight[0]) / float(ev.pairs[0])] and t["near_cluster"].tolist() == [-1] and len(ev.proximity(0)) == 0
    # two cliques apart: both complete; under the representatives' partition
    ev = _evaluation("cliques", "rep")
    t = ev.cluster_frame()
    assert t["complete"].tolist() == [True, True] and t["size"].tolist() == [cc.CLIQUE] * 2 and ev.complete().tolist() == [True, True]
    others = ev.size[ev.label].astype(np.float64) - 1.0
    assert ev.centrality().tobytes() == (ev.in_weight.astype(np.float64) / others).tobytes()
    g = ev.genome_frame()
    assert list(g.columns) == ["genome", "cluster", "medoid", "is_medoid", "centrality", "in_pairs", "in_weight", "in_min", "to_medoid", "out_pairs", "out_weight", "out_node"]
    assert g["genome"].tolist() == ev.labels and int(g["is_medoid"].sum()) == 2 and set(g["out_node"]) == {""}
    assert g["medoid"].tolist() == [ev.labels[m] for m in ev.medoid[ev.label].tolist()]
    # singletons: centrality 0.0, and the proximity table
    ev = _evaluation("random", "rep", labels=False)
    single = ev.size[ev.label] == 1
    assert single.any() and (ev.centrality()[single] == 0.0).all() and np.isfinite(ev.centrality()).all()
    t, p = ev.cluster_frame(), ev.proximity(4000)
    keep = ((t["near_cluster"] >= 0) & (t["near_weight"] >= 4000)).to_numpy()
    assert 0 < len(p) < len(t) and p["cluster"].tolist() == t["cluster"][keep].tolist() and (p["near_weight"] >= 4000).all()
    assert p["near_name"].tolist() == ev.naming()[p["near_cluster"].to_numpy()].tolist()
    assert (ev.naming()[t["near_cluster"][keep].to_numpy()] == ev.near_cluster[ev.naming()][keep]).all()
    assert len(ev.proximity(0)) == int((ev.near_cluster[ev.naming()] >= 0).sum())
    # an evaluation of nothing
    empty = screen.evaluation_from_nodes([], [], np.zeros(0, np.uint64), [np.zeros(0)] * 7, [np.zeros(0)] * 7)
    assert len(empty.genome_frame()) == 0 and len(empty.cluster_frame()) == 0 and len(empty.centrality()) == 0 and len(empty.recentred().size) == 0


@pytest.mark.parametrize("name,part", [("random", "rep"), ("random", "random"), ("cliques_joined", "root"), ("star", "rep"), ("self_entries", "root")])
def test_recentred_passes_the_clusters_own_validation(name, part):
    from pyani_amd import screen
    ev = _evaluation(name, part, labels=False)
    sc = ev.recentred()      # (clusters_from_nodes validates rep)
    assert isinstance(sc, screen.ScreenClusters) and (sc.rep == ev.medoid[ev.label]).all() and (sc.via == ev.to_medoid).all() and (sc.score == ev.score).all()
    assert sorted(sc.representative.tolist()) == sorted(ev.medoid[ev.naming()].tolist()) and (sc.via[sc.representative] == 0).all()
    same = screen.clusters_from_nodes(None, ev.label, np.zeros(len(ev.label), np.uint32), ev.score)
    assert sorted(sc.size.tolist()) == sorted(same.size.tolist())      # the clusters themselves do not change
    assert (ev.label[sc.rep] == ev.label).all()


def test_screened_pairs_evaluate_by_the_statement():
    from pyani_amd import screen
    a, b, s, n, label, score = ec.case("cliques_joined", "rep")
    sp = screen.ScreenedPairs([f"g{v}" for v in range(n)], screen.check_options(0.9), score.astype(np.uint32), a, b, s)
    ev = sp.evaluate(label)      # scores=None: the sizes
    ec.same((ev.node_arrays(), ev.cluster_arrays()), screen.evaluate_of_pairs(a, b, s, n, label, score.astype(np.uint32).astype(np.uint64)), "ScreenedPairs.evaluate")
    with pytest.raises(ValueError):
        sp.evaluate(label[:-1])
    with pytest.raises(ValueError):
        sp.evaluate(label, scores=[1.0])


def test_tables_written_and_read_back(tmp_path):
    from pyani_amd.subcmd_dereplicate import read_evaluation_tab, write_evaluation_tabs
    ev = _evaluation("random", "rep")
    write_evaluation_tabs(tmp_path / "genomes.tab", tmp_path / "clusters.tab", ev)
    for path, want in ((tmp_path / "genomes.tab", ev.genome_frame()), (tmp_path / "clusters.tab", ev.cluster_frame())):
        got = read_evaluation_tab(path)
        assert list(got.columns) == list(want.columns) and len(got) == len(want)
        for col in want.columns:
            if want[col].dtype == np.float64:      # repr's precision: the bits come back
                assert np.asarray(got[col], dtype=np.float64).tobytes() == want[col].to_numpy().tobytes(), col
            else:
                assert got[col].tolist() == want[col].tolist(), col


def test_run_dereplicate_refuses_an_unknown_winner_before_any_work(tmp_path):
    from pyani_amd.subcmd_dereplicate import DereplicateRun, EvaluatedDereplicateRun, run_dereplicate
    with pytest.raises(ValueError, match="winner"):
        run_dereplicate(tmp_path / "absent", screen=0.9, winner="best")
    # a run without an evaluation is the tuple it was; one with it carries it as an attribute beside the same eight fields
    plain = DereplicateRun({}, {}, None, None, (), None, [])
    assert plain.evaluation is None and plain.linkage is None
    with_it = EvaluatedDereplicateRun(*plain, evaluation="the evaluation")
    assert isinstance(with_it, DereplicateRun) and tuple(with_it) == tuple(plain) and with_it.evaluation == "the evaluation" and with_it.written == []
