"""CPU-only: the host side of the screen's index path — the band rule and the band ranges of pyani_amd/screen.py, the
stable-sort merge of dealt parts, the routing of path= and the ValueErrors of run_screen on a stub engine — and the index helpers of the
core header (pyani_amd/csrc/pg_screen_core.h) through a stand-alone sanitizer build (tests/screen/band_check.cpp)."""
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

SIZES = (1, 2, 8191, 8192, 8193, 65_536, 2 ** 20)


# ---- 1. bands ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_default_band_rule_and_ranges(n):
    from pyani_amd import screen
    rows = screen.default_band_rows(n)
    assert 1 <= rows <= min(8192, n) and rows * n <= 2 ** 29
    assert rows == min(8192, n) or (rows + 1) * n > 2 ** 29      # the largest such
    for setting in (0, 1 if n <= 8193 else 512, 3000, 8192):
        ranges = screen.band_ranges(n, setting)
        want_rows = setting or rows
        assert len(ranges) == -(-n // want_rows)
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))      # every row in exactly one band, the bands ascending
        assert all(r1 - r0 == want_rows for r0, r1 in ranges[:-1]) and 0 < ranges[-1][1] - ranges[-1][0] <= want_rows


def test_band_settings_outside_the_range_are_refused():
    from pyani_amd import screen
    assert screen.band_ranges(0) == []
    assert {n: screen.default_band_rows(n) for n in (8192, 65_536, 65_537, 2 ** 20)} == {8192: 8192, 65_536: 8192, 65_537: 8191, 2 ** 20: 512}
    with pytest.raises(ValueError):
        screen.band_ranges(10, 8193)
    with pytest.raises(ValueError):
        screen.band_ranges(10, -1)
    with pytest.raises(ValueError):
        screen.default_band_rows(0)
    assert screen.DENSE_MAX_GENOMES == screen.MAX_GENOMES == 8192 and screen.INDEX_MAX_GENOMES == 2 ** 20


# ---- 2. the merge of dealt parts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows,deal", [(50, 7, 3), (50, 7, 1), (64, 8, 4), (9, 1, 2), (30, 30, 3), (41, 5, 9)])
def test_merge_of_dealt_parts_is_the_single_list(n, rows, deal):
    from pyani_amd import screen
    rng = np.random.default_rng(n * 100 + rows)
    keep = rng.random((n, n)) < 0.2
    keep[rng.integers(0, n, 5)] = False      # rows that keep nothing
    a, b = np.nonzero(keep)
    s = rng.integers(0, 2 ** 32, len(a), dtype=np.uint64).astype(np.uint32)
    ranges = screen.band_ranges(n, rows)
    parts = []
    for d in range(deal):      # part d: the bands d, d + deal, ... in ascending order, each row-major
        idx = np.concatenate([np.flatnonzero((a >= r0) & (a < r1)) for r0, r1 in ranges[d::deal]] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        parts.append((a[idx].astype(np.int32), b[idx].astype(np.int32), s[idx]))
    assert sum(len(p[0]) for p in parts) == len(a)
    got = screen.merge_dealt(parts)
    assert [x.dtype for x in got] == [np.int32, np.int32, np.uint32]
    assert (got[0] == a).all() and (got[1] == b).all() and (got[2] == s).all()
    assert [len(x) for x in screen.merge_dealt([])] == [0, 0, 0]


# ---- 3. routing on a stub engine --------------------------------------------------------------------------------------------------------------
class StubEngine:
    """The screen calls of an Engine, recorded: every genome has 100 k-mers and shares 90 with its neighbours."""

    def __init__(self):
        from pyani_amd.engine import Engine
        self.calls = []
        self.screen_candidates = lambda *a, **kw: Engine.screen_candidates(self, *a, **kw)

    def _shared(self, n):
        m = np.zeros((n, n), dtype=np.uint32)
        i = np.arange(n - 1)
        m[i, i + 1] = m[i + 1, i] = 90
        m[np.arange(n), np.arange(n)] = 100
        return m

    def screen_hold(self, ids, kmer, scale):
        self.calls.append("hold")
        self.n = len(ids)
        return np.full(len(ids), 100, dtype=np.uint32)

    def screen_select(self, need):
        self.calls.append("select")
        from tests.screen_select_cases import rule
        return rule(self._shared(self.n), need)

    def screen_release(self):
        self.calls.append("release")

    def screen_index(self, ids, kmer, scale):
        self.calls.append("index")
        self.n = len(ids)
        return np.full(len(ids), 100, dtype=np.uint32)

    def screen_index_select(self, need, band_first=0, band_step=1):
        self.calls.append(("index_select", band_first, band_step))
        from tests.screen_select_cases import rule
        return rule(self._shared(self.n), need)

    def screen_index_release(self):
        self.calls.append("index_release")

    # the genome store and the dense matrix of run_screen
    def genome_count(self):
        return 0

    def add_fasta_batch(self, paths):
        return [(i, 1000 + i, 1) for i, _ in enumerate(paths)]

    def clear_genomes(self):
        self.calls.append("clear")

    def screen_matrix(self, ids, kmer=16, scale=256):
        self.calls.append("matrix")
        return np.full(len(ids), 100, dtype=np.uint32), self._shared(len(ids))


def test_path_routing(monkeypatch):
    from pyani_amd import screen
    ids = list(range(6))
    want = [(a, b) for a in range(6) for b in range(6) if abs(a - b) == 1]
    for path, calls in (("dense", ["hold", "select", "release"]), ("auto", ["hold", "select", "release"]),
                        ("index", ["index", ("index_select", 0, 1), "index_release"])):
        e = StubEngine()
        sp = e.screen_candidates(ids, 0.9, path=path)
        assert e.calls == calls and sp.pairs() == want and sp.options == screen.ScreenOptions(0.9) and (sp.shared == 90).all()
    assert StubEngine().screen_candidates(ids, 0.9).pairs() == want      # the default is "auto"
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 5)      # read at call time
    e = StubEngine()
    assert e.screen_candidates(ids, 0.9).pairs() == want and e.calls[0] == "index"
    e = StubEngine()
    assert e.screen_candidates(ids[:5], 0.9).pairs() == want[:8] and e.calls[0] == "hold"
    e = StubEngine()
    assert e.screen_candidates(ids, 0.9, path="dense").pairs() == want and e.calls[0] == "hold"      # an explicit path is taken as given
    with pytest.raises(ValueError, match="path"):
        StubEngine().screen_candidates(ids, 0.9, path="sparse")
    assert StubEngine().screen_candidates([], 0.9, path="index").pairs() == []

    class Failing(StubEngine):
        def screen_index_select(self, need, band_first=0, band_step=1):
            raise RuntimeError("select failed")
    e = Failing()
    with pytest.raises(RuntimeError):
        e.screen_candidates(ids, 0.9, path="index")
    assert e.calls == ["index", "index_release"]      # released on errors too


def test_index_path_takes_more_genomes_than_the_dense_one():
    from pyani_amd import screen
    ids = list(range(8193))
    e = StubEngine()
    with pytest.raises(ValueError, match="8192"):
        e.screen_candidates(ids, 0.9, path="dense")
    assert e.calls == []

    class Cheap(StubEngine):      # (no n x n array for 8193 genomes on the host)
        def screen_index_select(self, need, band_first=0, band_step=1):
            self.calls.append("index_select")
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
    e = Cheap()
    assert e.screen_candidates(ids, 0.9).pairs() == [] and e.calls == ["index", "index_select", "index_release"]
    with pytest.raises(ValueError, match=str(2 ** 20)):
        screen.index_candidates_on([e], lambda fn: [fn(e, 0)], range(2 ** 20 + 1), 0.9)


def test_dealing_over_several_engines():
    from pyani_amd import screen
    n = 7

    class Dealt(StubEngine):
        def __init__(self, k):
            super().__init__()
            self.k = k

        def screen_index_select(self, need, band_first=0, band_step=1):
            assert (band_first, band_step) == (self.k, 3)
            a, b, s = super().screen_index_select(need)
            mine = np.isin(a, [r for r0, r1 in screen.band_ranges(n, 2)[band_first::band_step] for r in range(r0, r1)])
            return a[mine], b[mine], s[mine]
    engines = [Dealt(k) for k in range(3)]
    sp = screen.index_candidates_on(engines, lambda fn: [fn(e, k) for k, e in enumerate(engines)], range(n), 0.9)
    assert sp.pairs() == [(a, b) for a in range(n) for b in range(n) if abs(a - b) == 1]
    assert all(e.calls[-1] == "index_release" for e in engines)


def test_run_screen_routing_and_errors(tmp_path, monkeypatch):
    from pyani_amd import screen
    from pyani_amd.subcmd_screen import ScreenRun, run_screen, tab_path
    indir = tmp_path / "in"
    indir.mkdir()
    for i in range(6):
        (indir / f"g{i}.fna").write_text(f">g{i}\nACGT\n")
    assert ScreenRun({}, None).screened is None      # the trailing field has a default
    e = StubEngine()
    run = run_screen(indir, engine=e)      # as before: the dense frames, no selection
    assert run.result is not None and run.screened is None and e.calls == ["matrix", "clear"]
    e = StubEngine()
    run = run_screen(indir, tmp_path / "out", engine=e, min_identity=0.9, write_output=True)
    assert run.result is not None and e.calls == ["matrix", "hold", "select", "release", "clear"]
    assert [(run.screened.labels[a], run.screened.labels[b]) for a, b in run.screened.pairs()][:2] == [("g0", "g1"), ("g1", "g0")]
    assert tab_path(tmp_path / "out", "pairs").read_text().splitlines()[1].split("\t")[:3] == ["g0", "g1", "90"]
    assert tab_path(tmp_path / "out", "shared").exists()
    monkeypatch.setattr(screen, "DENSE_MAX_GENOMES", 4)
    e = StubEngine()
    with pytest.raises(ValueError, match="min_identity"):
        run_screen(indir, engine=e)
    assert e.calls == []      # before any work
    run = run_screen(indir, tmp_path / "out2", engine=e, min_identity=0.9, write_output=True)
    assert run.result is None and len(run.screened.a) == 10 and e.calls == ["index", ("index_select", 0, 1), "index_release", "clear"]
    assert tab_path(tmp_path / "out2", "pairs").exists() and not tab_path(tmp_path / "out2", "shared").exists()
    assert tab_path(tmp_path / "out2", "pairs").read_text() == tab_path(tmp_path / "out", "pairs").read_text()
    with pytest.raises(ValueError):
        run_screen(indir, engine=StubEngine(), min_identity=float("nan"))
    with pytest.raises(ValueError):
        run_screen(indir, engine=StubEngine(), min_identity="0.8")


# ---- 4. the core header's index helpers on the host, under sanitizers ------------------------------------------------------------------------
def test_core_header_band_helpers_under_sanitizers(tmp_path):
    src = ROOT / "tests" / "screen" / "band_check.cpp"
    exe = tmp_path / "band_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "WRONG" not in out.stdout and out.stdout.count("ok ") == 4, out.stdout + out.stderr
    assert "ok default 21008" in out.stdout      # 20 000 + 7 + 1001 sizes


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree_on_the_index_calls():
    import re
    from pyani_amd import _lib, build
    build.build_gpu()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    for sym, arity in (("pg_screen_index", 6), ("pg_screen_index_release", 1), ("pg_screen_set_band", 2), ("pg_screen_index_select", 6),
                       ("pg_screen_index_read", 4), ("pg_screen_index_band", 3), ("pg_screen_index_last", 3)):
        decl = re.search(rf"\bint\s+{sym}\s*\(([^)]*)\)", text)
        assert decl and len(decl.group(1).split(",")) == arity, sym
        assert len(_lib.SIGNATURES[sym][1]) == arity and hasattr(lib, sym), sym
