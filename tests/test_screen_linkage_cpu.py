"""CPU-only: the STATEMENT of the linkage (pyani_amd.screen.linkage_of_pairs) against scipy per component
(tests/screen_linkage_cases.by_scipy: matrices from dicts, scipy's linkage and fcluster, a plain walk for the representatives), the
whole-matrix property, and the host code around it (ScreenLinkage, linkage_edges, run_dereplicate's argument checks).  Integers are
EQUAL and doubles bit for bit: no tolerance anywhere."""
import inspect

import numpy as np
import pytest

from pyani_amd import graphics, screen
from tests import screen_linkage_cases as lc
from tests.heatmap_cases import same_bits


def _same_nodes(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("root", "cluster", "rep")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("name,method,cutoff,fill,kind", lc.RUNS)
def test_statement_equals_scipy_per_component(name, method, cutoff, fill, kind):
    a, b, dist, n = lc.CASES[name]()
    score = lc.scores(kind, n)
    got = lc.expected(name, method, cutoff, fill, kind)
    root, cluster, rep, Zs = lc.by_scipy(a, b, dist, n, score, method, cutoff, fill)
    _same_nodes(got, (root, cluster, rep), (name, method))
    merges = got[3]
    assert merges.dtype == np.float64 and merges.shape == (n - len(np.unique(root)), 4)
    at = 0
    for Z in Zs:      # the blocks in ascending root order
        block = merges[at:at + len(Z)]
        assert same_bits(graphics.merges_to_linkage(block), Z), (name, method, at)
        at += len(Z)
    assert at == len(merges)
    if name == "quantised" and method == "complete":
        assert cutoff in set(merges[:, 2].tolist())      # the cutoff IS a height: <= must keep it
        assert len(set(merges[:, 2].tolist())) < len(merges) // 4      # ties everywhere
    if kind == "reversed" and name != "duplicates":
        assert (rep != cluster).sum() > 0      # a representative that is not its cluster's label


def test_linkage_of_matches_scipy_form():
    name, method, cutoff, fill, kind = lc.RUNS[0]
    a, b, dist, n = lc.CASES[name]()
    score = lc.scores(kind, n)
    L = screen.linkage_from_nodes(None, *lc.expected(name, method, cutoff, fill, kind)[:3], score, lc.expected(name, method, cutoff, fill, kind)[3], method, cutoff, fill)
    root, _, _, Zs = lc.by_scipy(a, b, dist, n, score, method, cutoff, fill)
    big = [r for r in np.unique(root).tolist() if (root == r).sum() >= 2]
    assert len(big) == len(Zs) == 9
    for r, Z in zip(big, Zs):
        got, members = L.linkage_of(r)
        assert same_bits(got, Z) and members.tolist() == np.flatnonzero(root == r).tolist()
    single = [r for r in np.unique(root).tolist() if (root == r).sum() == 1][0]
    assert L.linkage_of(single)[0].shape == (0, 4)
    with pytest.raises(IndexError):
        L.linkage_of(int(np.flatnonzero(root != np.arange(n))[0]))
    t = L.clusters()
    assert (t.via == 0).all() and (t.rep == L.rep).all() and len(t.size) == len(np.unique(L.cluster))
    f = L.frame()
    assert list(f.columns) == ["cluster", "representative", "size", "score", "component"] and len(f) == len(t.size)
    mf = L.merges_frame()
    assert len(mf) == len(L.merges) and mf["height"].tolist() == np.concatenate(Zs)[:, 2].tolist()


@pytest.mark.parametrize("method", screen.LINKAGE_METHODS)
@pytest.mark.parametrize("seed", range(6))
def test_partition_equals_one_linkage_over_the_whole_matrix(method, seed):
    """The property DESIGN.md §16.11 documents: absent pairs sit exactly at `fill` and cutoff < fill, so cutting the components' trees
    gives the partition of fcluster on ONE linkage over the n x n matrix.  Tie-free random cases, n <= 150."""
    rng = np.random.default_rng(100 + seed)
    sizes = rng.integers(1, 30, rng.integers(3, 8))
    sizes = sizes[:max(1, int(np.searchsorted(np.cumsum(sizes), 150, side="right")))]
    a, b, dist, n = lc.graph(sizes, 200 + seed, chords=1.5)
    assert n <= 150 and len(set(dist.tolist())) == len(dist)
    for cutoff in (0.05, 0.15, 0.29):
        _, cluster, _, _ = screen.linkage_of_pairs(a, b, dist, n, lc.scores("index", n), method=method, cutoff=cutoff, fill=1.0)
        assert (cluster == lc.whole_matrix_partition(a, b, dist, n, method, cutoff, 1.0)).all(), (seed, cutoff)


def test_order_direction_duplication_and_self_entries_do_not_matter():
    name, method, cutoff, fill, kind = "few", "average", 0.12, 1.0, "reversed"
    a, b, dist, n = lc.CASES[name]()
    score = lc.scores(kind, n)
    want = lc.expected(name, method, cutoff, fill, kind)

    def check(x, y, d, what):
        got = screen.linkage_of_pairs(x, y, d, n, score, method=method, cutoff=cutoff, fill=fill)
        _same_nodes(got, want, what)
        assert same_bits(got[3], want[3]), what
    order = np.random.default_rng(5).permutation(len(a))
    check(a[order], b[order], dist[order], "shuffled")
    check(b, a, dist, "reversed")
    check(np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([dist, dist]), "doubled")
    # a duplicate with a SMALLER distance changes nothing (the max rule); a self-entry is ignored whatever its distance
    selfs = np.arange(0, n, 3, dtype=np.int32)
    check(np.concatenate([a, b[:20], selfs]), np.concatenate([b, a[:20], selfs]), np.concatenate([dist, dist[:20] * 0.5, np.full(len(selfs), 0.9)]), "smaller duplicates")


def test_the_max_rule_on_duplicates():
    a, b, dist, n = lc.duplicates()
    root, cluster, rep, merges = screen.linkage_of_pairs(a, b, dist, n, lc.scores("constant", n), method="average", cutoff=0.05, fill=1.0)
    assert root.tolist() == [0, 0, 0, 3, 3, 5] and len(merges) == 3
    # the component {0, 1, 2}: D01 = 0.07 (not 0.02 or 0.04), D12 = 0.03, D02 = fill; {3, 4}: -0.0 and 0.0 give +0.0
    assert merges[0].tolist() == [1.0, 2.0, 0.03, 2.0]
    assert merges[1].tolist() == [0.0, 2.0, (1.0 * 0.07 + 1.0 * 1.0) / 2.0, 3.0]
    assert merges[2].tolist() == [0.0, 1.0, 0.0, 2.0] and not np.signbit(merges[2, 2])
    assert cluster.tolist() == [0, 1, 1, 3, 3, 5] and rep.tolist() == [0, 1, 1, 3, 3, 5]


def test_value_errors():
    a, b, dist, n = lc.duplicates()
    score = lc.scores("constant", n)
    ok = dict(method="average", cutoff=0.05, fill=1.0)
    for bad in (dist.astype(np.float32), np.where(dist == 0.5, np.nan, dist), np.where(dist == 0.5, np.inf, dist), np.where(dist == 0.5, -1e-9, dist), dist[:-1],
                [0] * len(a)):
        with pytest.raises(ValueError):
            screen.linkage_of_pairs(a, b, bad, n, score, **ok)
    for kw in (dict(method="single"), dict(method="ward"), dict(method=None), dict(cutoff=np.nan), dict(cutoff=-0.1), dict(cutoff=np.inf), dict(fill=np.inf),
               dict(fill=np.nan), dict(fill=-1.0), dict(cutoff=1.0), dict(cutoff=2.0), dict(cutoff=0.0, fill=0.0)):
        with pytest.raises(ValueError):
            screen.linkage_of_pairs(a, b, dist, n, score, **{**ok, **kw})
    for bad_n in (0, lc.MAX_N + 1, 3):
        with pytest.raises(ValueError):
            screen.linkage_of_pairs(a, b, dist, bad_n, np.zeros(max(bad_n, 0), np.uint64), **ok)
    with pytest.raises(ValueError):
        screen.linkage_of_pairs(a, b, dist, n, score[:-1], **ok)
    screen.linkage_of_pairs(a, b, dist, n, score, method="complete", cutoff=0.0, fill=1e-300)      # cutoff 0 is fine below any positive fill


def test_linkage_edges():
    """Both directions and the coverage are needed; the identity is not filtered; dist = 1 - the smaller identity."""
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_dereplicate import linkage_edges
    a = np.array([0, 1, 0, 2, 1, 2, 3, 0])
    b = np.array([1, 0, 2, 0, 2, 1, 0, 3])
    recs = np.zeros(len(a), dtype=Engine.ANIM_DTYPE)
    recs["identity"] = [0.99, 0.97, 0.6, 0.7, 0.9, 0.9, 0.99, 0.99]
    recs["ref_aln_len"] = [500, 500, 500, 500, 500, 50, 500, 500]      # (2, 1) covers 5 %: below 0.1
    recs["status"][7] = 1      # (0, 3): no alignment
    ea, eb, d = linkage_edges(a, b, recs, [1000, 1000, 1000, 1000], 0.1)
    assert d.dtype == np.float64 and sorted(zip(ea.tolist(), eb.tolist(), d.tolist())) == [(0, 1, 1.0 - 0.97), (0, 2, 1.0 - 0.6)]
    recs["status"][0] = -9
    with pytest.raises(RuntimeError):
        linkage_edges(a, b, recs, [1000] * 4, 0.1)


def test_run_dereplicate_argument_errors(tmp_path):
    """Every ValueError comes before any work: no engine is made (there is no device here) and the directory is never read."""
    from pyani_amd.subcmd_dereplicate import DereplicateRun, run_dereplicate
    missing = tmp_path / "nothing_here"
    for kw in (dict(secondary="single"), dict(secondary="ward"), dict(secondary=True), dict(secondary="average", cutoff=1.0), dict(secondary="average", cutoff=-0.01),
               dict(secondary="complete", cutoff=float("nan")), dict(secondary="average", exact="anim", min_ani=0.0), dict(secondary=None, cutoff=0.05),
               dict(secondary="average", exact="anib")):
        with pytest.raises(ValueError):
            run_dereplicate(missing, screen=0.9, **kw)
    assert DereplicateRun._fields[-1] == "linkage" and DereplicateRun._field_defaults == {"linkage": None}
    params = inspect.signature(run_dereplicate).parameters      # the greedy rule stays the default: nothing differs unless asked for
    assert params["secondary"].default is None and params["cutoff"].default is None and list(params)[-2:] == ["secondary", "cutoff"]
    assert 1.0 - 0.95 == 0.050000000000000044      # the default cutoff with exact="anim" is this float, unrounded
