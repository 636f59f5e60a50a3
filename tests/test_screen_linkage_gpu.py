"""GPU (through the C ABI): species clusters by linkage inside every component (pg_screen_linkage / _read / _read_merges / _set / _last /
_release; pyani_amd/csrc/pgscr_linkage.inc) against the numpy statement (pyani_amd.screen.linkage_of_pairs, itself held
to scipy by tests/test_screen_linkage_cpu.py).  Integers are EQUAL and doubles bit for bit, whatever the order of the list, the kernel a
component runs on, or the batches its matrices are worked in: no tolerance anywhere."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import screen_linkage_cases as lc
from tests import screen_representatives_cases as rc
from tests.heatmap_cases import same_bits

pytestmark = pytest.mark.gpu

NOTHING = {"n": 0, "entries": 0, "ignored": 0, "components": 0, "worked_components": 0, "largest": 0, "clusters": 0, "batches": 0,
           "group_ms": 0.0, "fill_ms": 0.0, "small_ms": 0.0, "large_ms": 0.0, "cut_ms": 0.0}


def _same(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("root", "cluster", "rep")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
    assert got[3].dtype == np.float64 and got[3].shape == want[3].shape, (what, got[3].shape, want[3].shape)
    if not same_bits(got[3], want[3]):
        rows = np.flatnonzero((got[3].view(np.uint64) != want[3].view(np.uint64)).any(axis=1))
        raise AssertionError((what, "merges", len(rows), rows[:3], got[3][rows[:3]], want[3][rows[:3]]))


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e
        e.screen_linkage_set(None, 0)


def _run(eng, name, method, cutoff, fill, kind):
    a, b, dist, n = lc.CASES[name]()
    return eng.screen_linkage(a, b, dist, n=n, score=lc.scores(kind, n), method=method, cutoff=cutoff, fill=fill)


@pytest.mark.parametrize("name,method,cutoff,fill,kind", lc.RUNS)
def test_list_equals_the_statement(eng, name, method, cutoff, fill, kind):
    """Among them: sizes (1, 2, 3, 31, 32, 33, 63, 64, 65 and 1025 nodes in one list: either side of the wave kernel's limits, one past a
    wave, one past the workgroup's threads), quantised (ties everywhere, a cutoff that is a height), many (5003 components of 2 ... 6),
    largest (n = 2^20, nearly all singletons), and every kind of scores (ties, unit scores, a representative that is not the label)."""
    eng.screen_linkage_set(None, 0)
    a, b, dist, n = lc.CASES[name]()
    want = lc.expected(name, method, cutoff, fill, kind)
    _same(_run(eng, name, method, cutoff, fill, kind), want, (name, method))
    last = eng.screen_linkage_last()
    live = int((a != b).sum())
    size = np.bincount(want[0], minlength=n)
    size = size[size > 0]
    assert (last["n"], last["entries"], last["ignored"]) == (n, live, len(a) - live), last
    assert (last["components"], last["worked_components"], last["largest"]) == (len(size), int((size >= 2).sum()), int(size.max())), last
    assert last["clusters"] == len(np.unique(want[1])) and last["batches"] == 1, last
    assert last["group_ms"] > 0.0 and last["fill_ms"] > 0.0 and last["cut_ms"] > 0.0
    assert (last["small_ms"] > 0.0) == bool(((size >= 2) & (size <= 32)).any()) and (last["large_ms"] > 0.0) == bool((size > 32).any()), last
    eng.screen_linkage_release()
    eng.screen_linkage_release()      # nothing resident: still fine
    assert eng.screen_linkage_last() == NOTHING


@pytest.mark.parametrize("small_limit", [0, 16, 32, 64])
@pytest.mark.parametrize("name,method,cutoff,fill,kind", [lc.RUNS[0], lc.RUNS[2], lc.RUNS[3], lc.RUNS[5]])
def test_every_small_limit_gives_the_same_bits(eng, small_limit, name, method, cutoff, fill, kind):
    """The wave kernel for components up to 16, 32, 64 nodes, or for none (0: the workgroup kernel does everything)."""
    try:
        eng.screen_linkage_set(small_limit, 0)
        _same(_run(eng, name, method, cutoff, fill, kind), lc.expected(name, method, cutoff, fill, kind), (name, method, small_limit))
        last = eng.screen_linkage_last()
        assert (last["small_ms"] > 0.0) == (small_limit > 0) and last["batches"] == 1, last
    finally:
        eng.screen_linkage_set(None, 0)
        eng.screen_linkage_release()


@pytest.mark.parametrize("small_limit", [0, 16, 32, 64])
@pytest.mark.parametrize("work_bytes,batches", [(8, 7), (8 * 40 * 40, 4), (8 * (40 * 40 + 4 + 81), 3)])
def test_batches_give_the_same_bits(eng, small_limit, work_bytes, batches):
    """`few` (components of 40, 2, 9, 33, 17, 5, 3 nodes in ascending root order of the scrambled labels) under budgets that put one
    component, or one or two, into a batch: a component beyond the budget has a batch to itself."""
    name, method, cutoff, fill, kind = lc.RUNS[6]
    want = lc.expected(name, method, cutoff, fill, kind)
    try:
        eng.screen_linkage_set(small_limit, work_bytes)
        _same(_run(eng, name, method, cutoff, fill, kind), want, (small_limit, work_bytes))
        last = eng.screen_linkage_last()
        assert last["worked_components"] == 7 and 2 <= last["batches"] <= 7, last
        if work_bytes == 8:
            assert last["batches"] == batches
    finally:
        eng.screen_linkage_set(None, 0)
        eng.screen_linkage_release()


def test_list_order_direction_and_duplication_do_not_matter(eng):
    name, method, cutoff, fill, kind = lc.RUNS[2]
    a, b, dist, n = lc.CASES[name]()
    score = lc.scores(kind, n)
    want = lc.expected(name, method, cutoff, fill, kind)
    kw = dict(n=n, score=score, method=method, cutoff=cutoff, fill=fill)
    order = np.random.default_rng(5).permutation(len(a))
    _same(eng.screen_linkage(a[order], b[order], dist[order], **kw), want, "shuffled")
    _same(eng.screen_linkage(b, a, dist, **kw), want, "reversed")
    _same(eng.screen_linkage(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([dist, dist]), **kw), want, "doubled")
    _same(eng.screen_linkage(np.concatenate([a, b[:50]]), np.concatenate([b, a[:50]]), np.concatenate([dist, dist[:50] * 0.5]), **kw), want, "smaller duplicates")
    eng.screen_linkage_release()


def test_capacity_refusals_and_release_leave_the_earlier_result(eng):
    from pyani_amd import _lib
    name, method, cutoff, fill, kind = lc.RUNS[7]
    a, b, dist, n = lc.CASES[name]()
    score = lc.scores(kind, n)
    want = lc.expected(name, method, cutoff, fill, kind)

    def refused(call, word, code=_lib.PG_E_ARG):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == code and word in str(err.value), str(err.value)

    def raw(x, y, d, nn, sc, m=_lib.PG_CLUSTER_AVERAGE, cut=0.1, fl=1.0):
        x, y, d = np.asarray(x, np.int32), np.asarray(y, np.int32), np.asarray(d, np.float64)
        c = ctypes.c_uint32(0)
        eng._check(eng.lib.pg_screen_linkage(eng._h, x.ctypes.data if len(x) else None, y.ctypes.data if len(x) else None, d.ctypes.data if len(x) else None, len(x), nn,
                                             None if sc is None else sc.ctypes.data, m, cut, fl, ctypes.byref(c)))
    eng.screen_linkage_release()
    eng.screen_linkage_release()
    assert eng.screen_linkage_last() == NOTHING
    refused(lambda: eng._screen_linkage_read(n), "no resident linkage")
    _same(eng.screen_linkage(a, b, dist, n=n, score=score, method=method, cutoff=cutoff, fill=fill), want, "before the refusals")
    before = eng.screen_linkage_last()
    z8 = np.zeros(8, np.uint64)
    calls = {
        "no node": (lambda: raw([], [], [], 0, z8), "nodes"), "too many nodes": (lambda: raw([], [], [], lc.MAX_N + 1, z8), "nodes"),
        "index below": (lambda: raw([-1], [3], [0.1], 8, z8), "outside"), "index at n": (lambda: raw([3], [8], [0.1], 8, z8), "outside"),
        "no score": (lambda: raw([1], [2], [0.1], 8, None), "score"), "nan": (lambda: raw([1], [2], [np.nan], 8, z8), "distance"),
        "inf": (lambda: raw([1], [2], [np.inf], 8, z8), "distance"), "negative": (lambda: raw([1], [2], [-0.5], 8, z8), "distance"),
        "method": (lambda: raw([1], [2], [0.1], 8, z8, m=2), "method"), "cutoff at fill": (lambda: raw([1], [2], [0.1], 8, z8, cut=1.0), "cutoff"),
        "cutoff nan": (lambda: raw([1], [2], [0.1], 8, z8, cut=np.nan), "cutoff"), "fill inf": (lambda: raw([1], [2], [0.1], 8, z8, fl=np.inf), "cutoff"),
        "cutoff negative": (lambda: raw([1], [2], [0.1], 8, z8, cut=-1.0), "cutoff"),
        "small limit": (lambda: eng.screen_linkage_set(65, 0), "small limit"), "work bytes": (lambda: eng.screen_linkage_set(32, (1 << 40) + 1), "bytes"),
    }
    for what, (call, word) in calls.items():
        refused(call, word)
        _same(eng._screen_linkage_read(n), want, ("after", what))      # still readable
        assert eng.screen_linkage_last() == before, what
    # one star of 8193 nodes: refused before any matrix is allocated (its 512 MiB would show in the time), the earlier result stays
    sa, sb, sd, sn = lc.star_beyond()
    refused(lambda: eng.screen_linkage(sa, sb, sd, n=sn, score=lc.scores("index", sn)), "8193", _lib.PG_E_CAPACITY)
    with pytest.raises(_lib.PyaniGpuError) as err:
        eng.screen_linkage(sa, sb, sd, n=sn, score=lc.scores("index", sn))
    assert "tighter screen threshold" in str(err.value)
    _same(eng._screen_linkage_read(n), want, "after the star")
    assert eng.screen_linkage_last() == before
    # independent of the components and the representatives: they come and go
    eng.screen_components(a, b, None, n=n)
    eng.screen_representatives(a, b, None, n=n, score=score)
    eng.screen_components_release()
    eng.screen_representatives_release()
    _same(eng._screen_linkage_read(n), want, "after the other states came and went")
    eng.screen_linkage_release()
    refused(lambda: eng._screen_linkage_read(n), "no resident linkage")
    # the Python entry refuses what the statement refuses, before the library is called
    for kw in (dict(method="single"), dict(cutoff=1.0), dict(fill=np.inf)):
        with pytest.raises(ValueError):
            eng.screen_linkage(a, b, dist, n=n, score=score, **kw)
    with pytest.raises(ValueError):
        eng.screen_linkage(a, b, dist.astype(np.float32), n=n, score=score)
    assert eng.screen_linkage_last() == NOTHING


def test_multi_engine_forwards_the_list_call(eng):
    from pyani_amd import multi
    name, method, cutoff, fill, kind = lc.RUNS[6]
    a, b, dist, n = lc.CASES[name]()
    m = multi.MultiEngine.__new__(multi.MultiEngine)
    m.engines = [eng]
    _same(m.screen_linkage(a, b, dist, n=n, score=lc.scores(kind, n), method=method, cutoff=cutoff, fill=fill), lc.expected(name, method, cutoff, fill, kind), "multi")
    assert m.screen_linkage_last()["n"] == n
    m.screen_linkage_release()
    assert eng.screen_linkage_last() == NOTHING


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
def test_run_dereplicate_secondary_on_three_families(eng, tmp_path):
    """The three families of the representatives' test (four genomes of 30 kb each, within a family less than 2 % apart): with
    secondary="average" every family is one cluster represented by its best score, with exact=None and with exact="anim"; the clusters
    are the statement's on the run's own edges; the files round-trip; and secondary=None writes what it wrote before, byte for byte."""
    from pyani_amd import screen
    from pyani_amd.subcmd_dereplicate import linkage_edges, read_linkage_tab, run_dereplicate, screen_linkage_edges
    from tests import fuzz_genomes
    indir = tmp_path / "genomes"
    indir.mkdir()
    for stem, seq in rc.family_genomes().items():
        fuzz_genomes.write_fasta(indir / f"{stem}.fna", stem, [seq])
    scores = rc.family_scores()
    stems = sorted(scores)
    best = sorted(s for s in stems if scores[s] == 100.0)
    score = screen.score_keys([scores[s] for s in stems])
    opt = screen.ScreenOptions(0.9, 16, 16)
    eng.clear_genomes()
    for exact in (None, "anim"):
        out = tmp_path / f"out_{exact}"
        run = run_dereplicate(indir, out, screen=opt, scores=scores, exact=exact, write_output=True, engine=eng, secondary="average")
        L = run.linkage
        assert L is not None and L.method == "average" and L.fill == 1.0
        assert L.cutoff == (1.0 - 0.95 if exact == "anim" else 1.0 - 0.9)      # the float the subtraction gives, unrounded
        assert run.clusters.labels == stems and run.representatives() == best, (exact, run.representatives())
        assert run.clusters.size.tolist() == [rc.PER_FAMILY] * rc.FAMILIES and (run.clusters.via == 0).all()
        if exact is None:
            assert run.records is None
            edges = screen_linkage_edges(run.screened)
        else:
            edges = linkage_edges(run.screened.a, run.screened.b, run.records, [run.lengths[s] for s in stems], 0.1)
            assert len(edges[0]) >= rc.FAMILIES * 6
        assert all(x.dtype == y.dtype and (x == y).all() for x, y in zip(edges, run.edges))
        want = screen.linkage_of_pairs(*edges, len(stems), score, method="average", cutoff=L.cutoff, fill=1.0)
        _same((L.root, L.cluster, L.rep, L.merges), want, exact)
        assert eng.genome_count() == 0 and eng.screen_linkage_last()["n"] == 0
        assert [p.name for p in run.written] == ["screen_pairs.tab", "screen_representatives.tab", "screen_clusters.tab", "screen_linkage.tab"]
        pd.testing.assert_frame_equal(pd.read_csv(run.written[1], sep="\t", dtype={"score": np.uint64}), run.clusters.frame())
        pd.testing.assert_frame_equal(pd.read_csv(run.written[2], sep="\t"), run.clusters.membership_frame())
        mf = L.merges_frame()
        rows = read_linkage_tab(run.written[3])
        assert len(rows) == len(L.merges) == len(stems) - len(np.unique(L.root))
        assert [r[0] for r in rows] == mf["component"].tolist() and [r[1:3] + r[4:] for r in rows] == list(zip(mf["left"], mf["right"], mf["size"]))
        assert same_bits([r[3] for r in rows], mf["height"].to_numpy())      # repr round-trips the bits
        # secondary=None: the fields and the files of the greedy rule, whether or not the keyword is named
        plain = run_dereplicate(indir, tmp_path / f"plain_{exact}", screen=opt, scores=scores, exact=exact, write_output=True, engine=eng)
        named = run_dereplicate(indir, tmp_path / f"named_{exact}", screen=opt, scores=scores, exact=exact, write_output=True, engine=eng, secondary=None)
        assert plain.linkage is None and named.linkage is None and len(plain.written) == len(named.written) == 3
        for p, q in zip(plain.written, named.written):
            assert p.name == q.name and p.read_bytes() == q.read_bytes()
        assert plain.representatives() == best
