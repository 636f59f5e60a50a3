"""CPU-only: the STATEMENT of the greedy representatives (pyani_amd.screen.representatives_of_pairs) against the
sequential walk of tests/screen_representatives_cases.py, its properties, and the host code around it (score_keys, clusters_from_nodes,
ScreenedPairs.representatives, run_dereplicate's argument checks).  Everything is an integer and must be EQUAL."""
import numpy as np
import pytest

from pyani_amd import screen
from tests import screen_components_cases as cc
from tests import screen_representatives_cases as rc


def _same(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.uint32), ("rep", "via")):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("name,kind", rc.PAIRS)
def test_statement_equals_the_walk(name, kind):
    a, b, s, n = cc.CASES[name]()
    _same(screen.representatives_of_pairs(a, b, s, n, rc.scores(kind, n)), rc.expected(name, kind), (name, kind))


@pytest.mark.parametrize("name,kind", [("random", "random"), ("cliques_joined_shuffled", "constant"), ("chain_scrambled", "random"), ("star", "reversed"),
                                       ("unweighted", "index")])
def test_properties(name, kind):
    a, b, s, n = cc.CASES[name]()
    score = rc.scores(kind, n)
    rep, via = screen.representatives_of_pairs(a, b, s, n, score)
    _, rank = screen.rank_order(score)
    is_rep = rep == np.arange(n)
    live = a != b
    a, b = a[live].astype(np.int64), b[live].astype(np.int64)
    w = np.ones(len(a), np.uint64) if s is None else s[live].astype(np.uint64)
    assert not (is_rep[a] & is_rep[b]).any()                       # an independent set
    assert (via[is_rep] == 0).all()
    # per covered node v, over the entries that join it to a representative: its own is among them with weight via, and none is better
    v = np.concatenate([b[is_rep[a] & ~is_rep[b]], a[is_rep[b] & ~is_rep[a]]])
    r = np.concatenate([a[is_rep[a] & ~is_rep[b]], b[is_rep[b] & ~is_rep[a]]])
    ww = np.concatenate([w[is_rep[a] & ~is_rep[b]], w[is_rep[b] & ~is_rep[a]]])
    assert set(np.flatnonzero(~is_rep).tolist()) == set(v.tolist())      # every other node has a representative neighbour (maximal)
    own = r == rep[v]
    best_own = np.zeros(n, np.uint64)
    np.maximum.at(best_own, v[own], ww[own])
    assert (best_own[~is_rep] == via[~is_rep]).all()               # adjacent to its rep, via = the maximum over the joining entries
    better = (ww > via[v]) | ((ww == via[v]) & (rank[r] < rank[rep[v]]))
    assert not better.any()                                        # no representative neighbour has a greater (weight, -rank)


@pytest.mark.parametrize("name,kind", [("random", "random"), ("cliques_joined", "index"), ("chain_shuffled", "reversed")])
def test_invariance(name, kind):
    a, b, s, n = cc.CASES[name]()
    score = rc.scores(kind, n)
    want = rc.expected(name, kind)
    order = np.random.default_rng(5).permutation(len(a))
    _same(screen.representatives_of_pairs(a[order], b[order], s[order], n, score), want, "shuffled")
    _same(screen.representatives_of_pairs(b, a, s, n, score), want, "reversed")
    _same(screen.representatives_of_pairs(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s]), n, score), want, "doubled")
    selfs = np.arange(0, n, 3, dtype=np.int32)
    _same(screen.representatives_of_pairs(np.concatenate([selfs, a]), np.concatenate([selfs, b]), np.concatenate([np.full(len(selfs), 2 ** 32 - 1, np.uint32), s]), n, score),
          want, "self-entries")


def test_assignment_after_the_walk_matters():
    a, b, w, n, score = rc.after_the_walk()
    rep, via = screen.representatives_of_pairs(a, b, w, n, score)
    assert rep.tolist() == [0, 2, 2] and via.tolist() == [0, 9, 0]      # the representative of LOWER priority than v takes v
    _same((rep, via), rc.walk(a, b, w, n, score), "the walk")
    assert rc.walk(a, b, w, n, score, assign_during_walk=True)[0].tolist() == [0, 0, 2]      # CD-HIT's form differs
    # ... and on the chains of the components' cases, as the docstring of the statement says
    ca, cb, cs, cn = cc.CASES["chain_ascending"]()
    cscore = rc.scores("random", cn)
    assert (rc.walk(ca, cb, cs, cn, cscore, assign_during_walk=True)[0] != rc.expected("chain_ascending", "random")[0]).any()


def test_refusals_of_the_statement():
    for bad_n, entry in cc.REFUSALS.values():
        x, y = ([], []) if entry is None else ([entry[0]], [entry[1]])
        with pytest.raises(ValueError):
            screen.representatives_of_pairs(x, y, None, bad_n, np.zeros(max(bad_n, 0), np.uint64))
    with pytest.raises(ValueError):
        screen.representatives_of_pairs([0], [1], None, 3, np.zeros(2, np.uint64))      # a score per node


def test_score_keys():
    x = np.array([0.0, -0.0, 5e-324, 1e-300, 0.5, 1.0, 1.0 + 2 ** -52, 3.0, 1e300])
    k = screen.score_keys(x)
    assert k.dtype == np.uint64 and k[0] == k[1] == 0      # -0.0 is 0.0
    assert (np.diff(k[1:].astype(object)) > 0).all()       # monotone: the order of the keys is the order of the doubles
    assert screen.score_keys([3, 1, 2]).argsort().tolist() == [1, 2, 0]
    for bad in ([-1.0], [float("nan")], [float("inf")], [1.0, -1e-300], ["x"]):
        with pytest.raises(ValueError):
            screen.score_keys(bad)
    sizes = np.array([7, 0, 2 ** 32 - 1], dtype=np.uint32)
    k = screen.score_keys(None, sizes)
    assert k.dtype == np.uint64 and k.tolist() == sizes.tolist()
    with pytest.raises(ValueError):
        screen.score_keys(None)


def test_clusters_from_nodes():
    a, b, s, n = cc.CASES["random"]()
    score = rc.scores("random", n)
    rep, via = rc.expected("random", "random")
    for labels in (None, [f"g{i}" for i in range(n)]):
        c = screen.clusters_from_nodes(labels, rep, via, score)
        assert int(c.size.sum()) == n and len(c.size) == len(c.representative) == int((rep == np.arange(n)).sum())
        assert (np.diff(c.representative) > 0).all() and (c.representative[c.cluster] == rep).all()
        assert c.start[0] == 0 and c.start[-1] == n and (np.diff(c.start) == c.size).all()
        for k in (0, len(c.size) - 1, int(c.size.argmax())):
            m = c.members(k)
            assert (np.diff(m) > 0).all() and (rep[m] == c.representative[k]).all() and len(m) == c.size[k]
        f, mf = c.frame(), c.membership_frame()
        assert list(f.columns) == ["cluster", "representative", "size", "score"] and len(f) == len(c.size)
        assert list(mf.columns) == ["genome", "representative", "via"] and len(mf) == n
        name = (lambda v: int(v)) if labels is None else (lambda v: labels[int(v)])
        assert c.representatives() == [name(v) for v in c.representative] == f["representative"].tolist()
        assert mf["representative"].tolist()[:50] == [name(v) for v in rep[:50]] and mf["via"].tolist() == via.tolist()
    empty = screen.clusters_from_nodes([], np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    assert len(empty.size) == 0 and empty.start.tolist() == [0] and len(empty.frame()) == 0
    with pytest.raises(ValueError):
        screen.clusters_from_nodes(None, [1, 0], [0, 0], [0, 0])      # rep[rep[v]] != rep[v]
    with pytest.raises(IndexError):
        screen.clusters_from_nodes(None, [0], [0], [0]).members(1)


def test_components_against_clusters():
    # a chain whose scores fall along it: ONE component, but every second node a representative
    a, b, s, n = cc.CASES["chain_ascending"]()
    assert int((cc.expected("chain_ascending")[0] == np.arange(n)).sum()) == 1
    rep, via = screen.representatives_of_pairs(a, b, s, n, rc.scores("index", n))
    assert int((rep == np.arange(n)).sum()) == 2048 and (rep[0::2] == np.arange(0, n, 2)).all()
    # two joined cliques: one component; node 0 represents its clique and covers node 300, the second clique's best of the rest stands
    a, b, s, n = cc.CASES["cliques_joined"]()
    assert int((cc.expected("cliques_joined")[0] == np.arange(n)).sum()) == 1
    rep, _ = screen.representatives_of_pairs(a, b, s, n, rc.scores("index", n))
    assert np.flatnonzero(rep == np.arange(n)).tolist() == [0, 301] and int((rep == np.arange(n)).sum()) == int((rc.expected("cliques_joined", "index")[0] == np.arange(n)).sum())
    # on cliques the two agree: a cluster per component, the same members
    a, b, s, n = cc.CASES["cliques"]()
    pairs = screen.ScreenedPairs([f"g{i}" for i in range(n)], screen.ScreenOptions(0.9), np.arange(n, dtype=np.uint32)[::-1].copy(), a, b, s)
    comps, clusters = pairs.components(), pairs.representatives()      # scores None: the sizes
    assert len(comps.size) == len(clusters.size) == 2 and (comps.component == clusters.cluster).all() and (comps.member == clusters.member).all()
    assert clusters.representatives() == ["g0", "g300"]
    given = pairs.representatives(scores=np.arange(n, dtype=np.float64))
    assert given.representatives() == ["g299", "g599"]
    with pytest.raises(ValueError):
        pairs.representatives(scores=np.zeros(3))


def test_run_dereplicate_refuses_before_an_engine_is_touched(tmp_path, monkeypatch):
    from pyani_amd import subcmd_dereplicate as sd

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(sd, "default_engine", no_engine)
    (tmp_path / "in").mkdir()
    for stem in ("x", "y"):
        (tmp_path / "in" / f"{stem}.fna").write_text(">r\nACGTACGTACGTACGTACGTACGT\n")
    with pytest.raises(ValueError, match="screen="):
        sd.run_dereplicate(tmp_path / "in")
    with pytest.raises(ValueError, match="output directory"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, write_output=True)
    with pytest.raises(ValueError, match="exact"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, exact="anib")
    with pytest.raises(ValueError, match="no genome of this run"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores={"x": 1.0, "y": 2.0, "z": 3.0})
    with pytest.raises(ValueError, match="no score"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores={"x": 1.0})
    with pytest.raises(ValueError, match="finite"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores={"x": 1.0, "y": -2.0})
    tsv = tmp_path / "scores.tsv"
    tsv.write_text("# stem\tscore\nx\t1.5\nq\t2\n")
    assert sd.read_scores(tsv) == {"x": 1.5, "q": 2.0}
    with pytest.raises(ValueError, match="no genome of this run"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores=tsv)
    tsv.write_text("x\tone\n")
    with pytest.raises(ValueError, match="no number"):
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores=tsv)
    with pytest.raises(AssertionError, match="an engine was asked for"):      # with sound arguments the engine is the next thing asked for
        sd.run_dereplicate(tmp_path / "in", screen=0.9, scores={"x": 1.0, "y": 2.0})


def test_exact_edges():
    from pyani_amd import subcmd_dereplicate as sd
    from pyani_amd.engine import Engine
    a, b = np.array([0, 1, 0, 2, 1, 2]), np.array([1, 0, 2, 0, 2, 1])
    recs = np.zeros(6, dtype=Engine.ANIM_DTYPE)
    recs["identity"] = [0.99, 0.97, 0.99, 0.94, 0.99, 0.99]       # 0-2: one direction below min_ani
    recs["ref_aln_len"] = [900, 800, 900, 900, 900, 50]           # 1-2: the coverage of query 2 is 0.05
    ea, eb, w = sd.exact_edges(a, b, recs, [1000, 1000, 1000], 0.95, 0.1)
    assert (ea.tolist(), eb.tolist(), w.tolist()) == ([0], [1], [970000])
    recs["status"][1] = 1      # no alignment: no result in that direction
    assert len(sd.exact_edges(a, b, recs, [1000, 1000, 1000], 0.95, 0.1)[0]) == 0
