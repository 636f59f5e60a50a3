"""CPU-only: the connected components of the screen's kept pairs (pyani_amd/screen.py) — the numpy statement against
two references that share nothing with it (tests/screen_components_cases.py: a union-find of the tests' own, and scipy), the derived
fields of ScreenComponents, its frames, merge_components on hand-cut parts, the drivers' routing on a stub engine, and the C ABI.
Everything is an integer and must be EQUAL."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import screen_components_cases as cc

ROOT = Path(__file__).resolve().parent.parent


def _same_nodes(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.uint64, np.uint64), ("root", "entries", "weight")):
        w = np.asarray(w)
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


# ---- 1. the statement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_statement_equals_the_union_find_and_scipy(name):
    from pyani_amd import screen
    a, b, s, n = cc.CASES[name]()
    got = screen.components_of_pairs(a, b, s, n)
    _same_nodes(got, cc.expected(name), name)
    roots, count = cc.scipy_roots(a, b, n)
    assert (got[0] == roots).all() and int((got[0] == np.arange(n)).sum()) == count
    live = a != b
    assert int(got[1].sum()) == int(live.sum())
    assert int(got[2].sum()) == (int(live.sum()) if s is None else int(s[live].astype(np.uint64).sum()))


def test_what_the_cases_are_made_for():
    from pyani_amd import screen
    root, entries, weight = cc.expected("random")
    sc = screen.components_from_nodes(None, root, entries, weight)
    assert len(sc.size) == cc.RANDOM_COMPONENTS == 20186 and int(sc.size.max()) == cc.RANDOM_LARGEST == 16106
    root, entries, weight = cc.expected("star")
    assert (root == 0).all() and entries[-1] == cc.STAR_LEAVES and entries[:-1].sum() == 0 and weight[-1] == 3 * cc.STAR_LEAVES
    root, entries, weight = cc.expected("largest")
    assert root[cc.MAX_N - 1] == 5 and root[700_000] == 5 and entries[cc.MAX_N - 1] == 2 and weight[cc.MAX_N - 1] == 6
    assert cc.expected("heavy")[2][2] == 3 * (2 ** 32 - 1) > 2 ** 32
    assert (cc.expected("self_entries")[0] == np.arange(5)).all() and cc.expected("self_entries")[1].sum() == 0
    _same_nodes(cc.expected("one_direction"), ([0, 0, 2], [0, 1, 0], [0, 5, 0]), "one direction")
    for shuffled in ("cliques_shuffled", "cliques_joined_shuffled"):      # the same list in another order: the same arrays
        _same_nodes(cc.expected(shuffled), cc.expected(shuffled.replace("_shuffled", "")), shuffled)
    for name in ("chain_ascending", "chain_descending", "chain_shuffled", "chain_scrambled"):
        assert (cc.expected(name)[0] == 0).all()


def test_statement_refuses():
    from pyani_amd import screen
    for n, entry in cc.REFUSALS.values():
        a, b = ([], []) if entry is None else ([entry[0]], [entry[1]])
        with pytest.raises(ValueError):
            screen.components_of_pairs(a, b, None, n)
    with pytest.raises(ValueError):
        screen.components_of_pairs([0, 1], [1], None, 3)
    with pytest.raises(ValueError):
        screen.components_of_pairs([0], [1], [1, 2], 3)


# ---- 2. the derived fields -------------------------------------------------------------------------------------------------------------------
def test_derived_fields_of_the_cliques():
    from pyani_amd import screen
    for name, complete in (("cliques", [True, True]), ("cliques_joined", [False])):
        sc = screen.components_from_nodes(None, *cc.expected(name))
        assert sc.complete.tolist() == complete and sc.complete.dtype == bool
        assert sc.size.tolist() == ([300, 300] if len(complete) == 2 else [600]) and int(sc.size.sum()) == 600
        assert sc.edges.dtype == np.uint64 and int(sc.edges.sum()) == 2 * 300 * 299 + (len(complete) == 1)
        assert sc.start.tolist() == np.concatenate([[0], np.cumsum(sc.size)]).tolist()
        for c in range(len(sc.size)):
            m = sc.members(c)
            assert (np.diff(m) > 0).all() and (sc.component[m] == c).all() and sc.root[m[0]] == m[0] and (sc.root[m] == m[0]).all()
            w = sc.weight[m]
            assert sc.representative[c] == m[np.flatnonzero(w == w.max())[0]]
    with pytest.raises(IndexError):
        sc.members(1)


def test_numbering_representatives_and_ties():
    from pyani_amd import screen
    #        node   0  1  2  3  4  5  6
    root = np.array([0, 1, 0, 3, 1, 3, 6], dtype=np.int32)      # {0, 2}, {1, 4}, {3, 5}, {6}
    entries = np.array([1, 1, 1, 2, 1, 0, 0], dtype=np.uint64)
    weight = np.array([5, 9, 5, 2 ** 40, 9, 2 ** 40 + 1, 0], dtype=np.uint64)
    labels = list("abcdefg")
    sc = screen.components_from_nodes(labels, root, entries, weight)
    assert sc.component.tolist() == [0, 1, 0, 2, 1, 2, 3] and sc.component.dtype == np.int32      # numbered by ascending root
    assert sc.member.tolist() == [0, 2, 1, 4, 3, 5, 6] and sc.start.tolist() == [0, 2, 4, 6, 7]
    assert sc.size.tolist() == [2, 2, 2, 1] and sc.edges.tolist() == [2, 2, 2, 0]
    assert sc.complete.tolist() == [True, True, True, True]      # a singleton: 0 == 1 x 0
    assert sc.representative.tolist() == [0, 1, 5, 6]      # ties to the smallest index; beyond 2^32 still by weight; a singleton itself
    assert sc.representatives() == ["a", "b", "f", "g"]
    assert [sc.members(c).tolist() for c in range(4)] == [[0, 2], [1, 4], [3, 5], [6]]
    f = sc.frame()
    assert list(f.columns) == ["component", "size", "representative", "edges", "complete"]
    assert f["component"].tolist() == [0, 1, 2, 3] and f["representative"].tolist() == ["a", "b", "f", "g"] and f["size"].tolist() == [2, 2, 2, 1]
    m = sc.membership_frame()
    assert list(m.columns) == ["genome", "component", "representative"]
    assert m["genome"].tolist() == labels and m["component"].tolist() == [0, 1, 0, 2, 1, 2, 3]
    assert m["representative"].tolist() == ["a", "b", "a", "f", "b", "f", "g"]
    assert screen.components_from_nodes(None, root, entries, weight).representatives() == [0, 1, 5, 6]      # no labels: the indices
    with pytest.raises(ValueError):
        screen.components_from_nodes(labels[:3], root, entries, weight)
    with pytest.raises(ValueError):      # 2 -> 1 -> 0 is not flattened
        screen.components_from_nodes(None, np.array([0, 0, 1], np.int32), np.zeros(3, np.uint64), np.zeros(3, np.uint64))
    empty = screen.components_from_nodes([], np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    assert len(empty.size) == 0 and empty.start.tolist() == [0] and len(empty.frame()) == 0 and empty.representatives() == []


def test_screened_pairs_components_without_an_engine():
    from pyani_amd import screen
    a, b, s, n = cc.CASES["cliques_joined"]()
    labels = [f"g{i}" for i in range(n)]
    sp = screen.ScreenedPairs(labels, screen.ScreenOptions(0.9), np.full(n, 5000, np.uint32), a, b, s)
    sc = sp.components()
    _same_nodes((sc.root, sc.entries, sc.weight), cc.expected("cliques_joined"), "ScreenedPairs.components")
    assert sc.labels == labels and len(sc.size) == 1 and not sc.complete[0]
    none = screen.ScreenedPairs([], screen.ScreenOptions(0.9), np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    assert len(none.components().size) == 0


# ---- 3. merging the forests of parts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "cliques_joined", "chain_scrambled", "one_direction"])
def test_merge_components_on_hand_cut_parts(name):
    from pyani_amd import screen
    a, b, s, n = cc.CASES[name]()
    whole = cc.expected(name)
    for n_parts in (1, 2, 3):
        parts = [screen.components_of_pairs(a[k::n_parts], b[k::n_parts], None if s is None else s[k::n_parts], n) for k in range(n_parts)]
        _same_nodes(screen.merge_components(parts, n), whole, (name, n_parts))
    # cut by the row, as dealt bands are: a part owns whole rows
    parts = [screen.components_of_pairs(a[a % 2 == k], b[a % 2 == k], None if s is None else s[a % 2 == k], n) for k in (0, 1)]
    _same_nodes(screen.merge_components(parts, n), whole, (name, "rows"))
    with pytest.raises(ValueError):
        screen.merge_components([tuple(x[:-1] for x in whole)], n)


# ---- 4. routing: what the drivers call, on an engine that only records ---------------------------------------------------------------------------
class StubEngine:
    """Six genomes in a row; the screen keeps the neighbours 0-1, 1-2 | 3-4 (both directions), 5 alone."""
    KEPT = [(0, 1), (1, 0), (1, 2), (2, 1), (3, 4), (4, 3)]

    def __init__(self):
        self.calls, self.n = [], 0

    def genome_count(self):
        return self.n

    def add_fasta_batch(self, paths):
        out = [(self.n + k, 4, 1) for k in range(len(paths))]
        self.n += len(paths)
        return out

    def clear_genomes(self):
        self.calls.append("clear")
        self.n = 0

    def screen_matrix(self, ids, kmer=16, scale=256, part=0, n_parts=1):
        self.calls.append("matrix")
        n = len(ids)
        shared = np.zeros((n, n), dtype=np.uint32)
        for x, y in self.KEPT:
            shared[x, y] = 90
        np.fill_diagonal(shared, 100)
        return np.full(n, 100, dtype=np.uint32), shared

    def _list(self):
        a, b = np.array(self.KEPT, dtype=np.int32).T
        return a, b, np.full(len(a), 90, dtype=np.uint32)

    def screen_candidates(self, ids, options, labels=None, path="auto"):
        from pyani_amd import screen
        self.calls.append(("candidates", path))
        return screen.ScreenedPairs([str(x) for x in (labels or ids)], screen.check_options(options), np.full(len(ids), 100, np.uint32), *self._list())

    def screen_components(self, a, b, shared=None, n=0):
        from pyani_amd import screen
        self.calls.append(("components", len(a), n))
        return screen.components_of_pairs(a, b, shared, n)

    def screen_index(self, ids, kmer=16, scale=256):
        self.calls.append("index")
        return np.full(len(ids), 100, dtype=np.uint32)

    def screen_index_components(self, need, band_first=0, band_step=1):
        from pyani_amd import screen
        self.calls.append(("index_components", band_first, band_step))
        a, b, s = self._list()
        mine = (a % band_step) == band_first      # a band of one row
        return (*screen.components_of_pairs(a[mine], b[mine], s[mine], len(need)), int(mine.sum()))

    def screen_index_release(self):
        self.calls.append("index_release")

    def screen_components_release(self):
        self.calls.append("components_release")

    def screen_components_of(self, ids, options, labels=None, path="auto"):
        from pyani_amd.engine import Engine
        return Engine.screen_components_of(self, ids, options, labels, path)


def test_components_of_routing(monkeypatch):
    from pyani_amd import screen
    ids = list(range(6))
    for path, calls in (("dense", [("candidates", "dense"), ("components", 6, 6), "components_release"]),
                        ("index", ["index", ("index_components", 0, 1), "index_release", "components_release"])):
        e = StubEngine()
        sc = e.screen_components_of(ids, 0.9, path=path)
        assert e.calls == calls, (path, e.calls)
        assert sc.root.tolist() == [0, 0, 0, 3, 3, 5] and sc.size.tolist() == [3, 2, 1] and sc.labels == [str(i) for i in ids]
        assert sc.complete.tolist() == [False, True, True] and sc.representative.tolist() == [1, 3, 5] and sc.edges.tolist() == [4, 2, 0]
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 5)      # "auto" follows resolve_path
    e = StubEngine()
    e.screen_components_of(ids, 0.9)
    assert e.calls[0] == "index"
    with pytest.raises(ValueError, match="path"):
        StubEngine().screen_components_of(ids, 0.9, path="sparse")
    assert len(StubEngine().screen_components_of([], 0.9, path="index").size) == 0

    class Failing(StubEngine):
        def screen_index_components(self, need, band_first=0, band_step=1):
            raise RuntimeError("failed")
    e = Failing()
    with pytest.raises(RuntimeError):
        e.screen_components_of(ids, 0.9, path="index")
    assert e.calls == ["index", "index_release", "components_release"]      # released on errors too


def test_dealt_parts_are_merged_on_the_first_engine():
    from pyani_amd import screen
    engines = [StubEngine() for _ in range(3)]
    sc = screen.index_components_on(engines, lambda fn: [fn(e, k) for k, e in enumerate(engines)], range(6), 0.9)
    assert sc.root.tolist() == [0, 0, 0, 3, 3, 5] and sc.entries.tolist() == [1, 2, 1, 1, 1, 0] and sc.weight.tolist() == [90, 180, 90, 90, 90, 0]
    assert [e.calls[1] for e in engines] == [("index_components", k, 3) for k in range(3)]
    assert engines[0].calls[2][0] == "components" and all("components" not in str(e.calls[2]) for e in engines[1:])      # the join: one list call
    assert all(e.calls[-2:] == ["index_release", "components_release"] for e in engines)


def test_run_screen_components(tmp_path):
    import pandas as pd
    from pyani_amd.subcmd_screen import ScreenRun, run_screen, tab_path
    indir = tmp_path / "in"
    indir.mkdir()
    for i in range(6):
        (indir / f"g{i}.fna").write_text(f">g{i}\nACGT\n")
    assert ScreenRun({}, None).components is None and ScreenRun._fields[:3] == ("lengths", "result", "screened")
    # components=False: the calls, the result and the files of before
    e = StubEngine()
    plain = run_screen(indir, tmp_path / "plain", engine=e, min_identity=0.9, write_output=True)
    assert e.calls == ["matrix", ("candidates", "auto"), "clear"] and plain.components is None
    assert sorted(p.name for p in (tmp_path / "plain" / "screen_output").iterdir()) == [f"screen_{x}.tab" for x in ("containment", "identity", "pairs", "shared")]
    e = StubEngine()
    run = run_screen(indir, tmp_path / "out", engine=e, min_identity=0.9, write_output=True, components=True)
    assert e.calls == ["matrix", ("candidates", "auto"), ("components", 6, 6), "components_release", "clear"]
    assert (run.result.shared == plain.result.shared).all() and run.screened.pairs() == plain.screened.pairs() and run.lengths == plain.lengths
    assert run.components.labels == [f"g{i}" for i in range(6)] and run.components.representatives() == ["g1", "g3", "g5"]
    comp = pd.read_csv(tab_path(tmp_path / "out", "components"), sep="\t")
    assert list(comp.columns) == ["component", "size", "representative", "edges", "complete"]
    assert comp["size"].tolist() == [3, 2, 1] and comp["representative"].tolist() == ["g1", "g3", "g5"] and comp["complete"].tolist() == [False, True, True]
    mem = pd.read_csv(tab_path(tmp_path / "out", "membership"), sep="\t")
    assert list(mem.columns) == ["genome", "component", "representative"] and mem["component"].tolist() == [0, 0, 0, 1, 1, 2]
    assert tab_path(tmp_path / "out", "pairs").read_bytes() == tab_path(tmp_path / "plain", "pairs").read_bytes()
    e = StubEngine()
    with pytest.raises(ValueError, match="min_identity"):
        run_screen(indir, engine=e, components=True)
    assert e.calls == []      # before any work


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree_on_the_components_calls():
    from pyani_amd import _lib, build
    build.build_gpu()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    for sym, arity in (("pg_screen_components", 7), ("pg_screen_index_components", 7), ("pg_screen_components_read", 4),
                       ("pg_screen_components_last", 3), ("pg_screen_components_release", 1)):
        decl = re.search(rf"\bint\s+{sym}\s*\(([^)]*)\)", text)
        assert decl and len(decl.group(1).split(",")) == arity, sym
        assert len(_lib.SIGNATURES[sym][1]) == arity and hasattr(lib, sym), sym
    from pyani_amd import subcmd_components
    assert callable(subcmd_components.run_anim_components)
