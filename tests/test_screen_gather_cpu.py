"""CPU: the host side of the screen's gather — the statement of tests/screen_gather_cases.py against a brute-force
re-count over an incidence matrix, ties included; gather_thresholds and GatherOptions; the frame and the summary of a GatherResult; the
calls declared, bound and exported; Engine.screen_gather on a stub library (chunks, and the release on errors).  No device."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import screen_gather_cases as sgc

ROOT = Path(__file__).resolve().parent.parent
CALLS = ("pg_screen_gather_count", "pg_screen_gather", "pg_screen_gather_read", "pg_screen_gather_fetch", "pg_screen_gather_last", "pg_screen_gather_matched")


def _brute(query_sets, db_sets, need, max_ranks):
    """The same rounds over a 0/1 incidence matrix (db x universe) and a mask of the query's remaining k-mers: another route to the rows."""
    universe = sorted(set().union(*[set(s) for s in db_sets], *[set(s) for s in query_sets]))
    at = {x: j for j, x in enumerate(universe)}
    inc = np.zeros((len(db_sets), len(universe)), dtype=np.int64)
    for b, s in enumerate(db_sets):
        inc[b, [at[x] for x in s]] = 1
    rows, lefts = [], []
    for i, s in enumerate(query_sets):
        mask = np.zeros(len(universe), dtype=np.int64)
        mask[[at[x] for x in s]] = 1
        total = inc @ mask
        rank = 0
        while rank < max_ranks:
            left = inc @ mask
            w = int(np.argmax(left))      # (the first of the largest: the smallest b)
            if left[w] < need[i]:
                break
            rows.append((i, w, int(left[w]), int(total[w])))
            mask = mask * (1 - inc[w])
            rank += 1
        lefts.append(inc @ mask)
    return rows, np.array(lefts, dtype=np.uint32).reshape(len(query_sets), len(db_sets))


@pytest.mark.parametrize("seed", range(6))
def test_the_statement_is_the_brute_force_recount(seed):
    rng = np.random.default_rng(seed)
    n, q, universe = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(4, 40))
    db = [sorted(rng.choice(universe, size=int(rng.integers(0, universe)), replace=False).tolist()) for _ in range(n)]
    if n >= 3:
        db[2] = list(db[0])      # a tie of whole genomes
    queries = [sorted(rng.choice(universe + 5, size=int(rng.integers(0, universe)), replace=False).tolist()) for _ in range(q)]
    for need, max_ranks in ((1, 65536), (3, 65536), (1, 2)):
        g = sgc.gather_sets(queries, db, [need] * q, max_ranks)
        rows, left = _brute(queries, db, [need] * q, max_ranks)
        assert list(zip(g.query.tolist(), g.db.tolist(), g.unique.tolist(), g.total.tolist())) == rows, (seed, need, max_ranks)
        assert np.array_equal(g.left, left)
        sgc.check_consequences(g, n, max_ranks)
        # what was explained plus what stayed = what matched the collection at all
        union = set().union(*[set(s) for s in db])
        for i in range(q):
            explained = int(g.unique[g.query == i].sum())
            taken = set().union(set(), *[set(db[w]) for w in g.db[g.query == i].tolist()])
            assert explained + len((set(queries[i]) & union) - taken) == g.matched[i] == len(set(queries[i]) & union)
        assert g.claimed == int(g.unique.sum()) and g.decrements >= g.claimed


def test_ties_go_to_the_smaller_index():
    db = [[1, 2, 3], [1, 2, 3], [3, 4], [5]]
    g = sgc.gather_sets([[1, 2, 3, 4, 5, 9]], db, [1], 65536)
    assert g.db.tolist() == [0, 2, 3] and g.unique.tolist() == [3, 1, 1] and g.total.tolist() == [3, 2, 1]
    assert g.left.tolist() == [[0, 0, 0, 0]] and g.matched.tolist() == [5]
    assert g.claimed == 5 and g.decrements == 3 * 2 + 1 + 1 + 1 and g.rounds == 4      # k-mer 3 has three holders, 1 and 2 two each
    assert sgc.gather_sets([[1, 2, 3, 4, 5, 9]], db, [2], 65536).db.tolist() == [0]
    assert sgc.gather_sets([[1, 2, 3, 4, 5, 9]], db, [1], 2).db.tolist() == [0, 2]
    none = sgc.gather_sets([], db, [], 5)
    assert len(none.query) == 0 and none.rounds == 0 and none.left.shape == (0, 4)


def test_gather_thresholds():
    from pyani_amd import screen
    t = screen.gather_thresholds([0, 1, 99, 100, 101, 4_000_000_000], 3, 0.05)
    assert t.dtype == np.uint32 and t.tolist() == [3, 3, 5, 5, 6, 200_000_000]
    assert screen.gather_thresholds([0, 10, 1000], 0, 0.0).tolist() == [1, 1, 1]      # floored at 1
    assert screen.gather_thresholds([7, 8], 2, 1.0).tolist() == [7, 8]
    assert screen.gather_thresholds([], 5).tolist() == []
    for bad in ((-1, 0.0), (1.5, 0.0), (True, 0.0), (1, -0.1), (1, 1.5), (1, float("nan")), (1 << 32, 0.0)):
        with pytest.raises(ValueError):
            screen.gather_thresholds([10], *bad)


def test_gather_options():
    from pyani_amd import screen
    o = screen.check_gather_options(screen.GatherOptions(16, 256, 50))
    assert o == screen.GatherOptions(16, 256, 50, 0.0, 65536) and isinstance(o.min_fraction, float)
    assert screen.check_gather_options(screen.GatherOptions(np.int64(12), 16, np.int32(1), 1, 7)) == screen.GatherOptions(12, 16, 1, 1.0, 7)
    for bad in (screen.GatherOptions(7, 256, 5), screen.GatherOptions(16, 3, 5), screen.GatherOptions(16, 256, 0), screen.GatherOptions(16, 256, 2.5),
                screen.GatherOptions(16, 256, True), screen.GatherOptions(16, 256, 5, -0.1), screen.GatherOptions(16, 256, 5, 2.0),
                screen.GatherOptions(16, 256, 5, float("nan")), screen.GatherOptions(16, 256, 5, 0.0, 0), screen.GatherOptions(16, 256, 5, 0.0, 65537),
                screen.GatherOptions(16, 256, 5, 0.0, 1.0), 0.9, None, screen.ScreenOptions(0.9)):
        with pytest.raises(ValueError):
            screen.check_gather_options(bad)


def _result(k=16):
    from pyani_amd import screen
    return screen.GatherResult(["q0", "q1", "q2"], ["d0", "d1", "d2"], screen.GatherOptions(k, 16, 1), np.array([100, 0, 40], np.uint32),
                               np.array([200, 50, 0], np.uint32), np.array([0, 0, 2], np.int32), np.array([1, 0, 1], np.int32),
                               np.array([30, 20, 10], np.uint32), np.array([30, 45, 10], np.uint32), np.array([60, 0, 10], np.uint32))


def test_gather_result_frame_and_summary():
    r = _result()
    f = r.frame()
    assert list(f.columns) == ["query", "rank", "db", "unique", "total", "f_unique_query", "f_unique_cumulative", "f_match", "identity"]
    assert list(f["query"]) == ["q0", "q0", "q2"] and list(f["db"]) == ["d1", "d0", "d1"] and list(f["rank"]) == [0, 1, 0]
    assert list(f["unique"]) == [30, 20, 10] and list(f["total"]) == [30, 45, 10]
    assert np.array_equal(f["f_unique_query"].to_numpy(), [30 / 100, 20 / 100, 10 / 40])
    assert np.array_equal(f["f_unique_cumulative"].to_numpy(), [30 / 100, 50 / 100, 10 / 40])      # the running sum starts again with every query
    assert np.array_equal(f["f_match"].to_numpy(), [30 / 50, 45 / 200, 10 / 50])
    assert np.array_equal(f["identity"].to_numpy(), np.power(np.array([30 / 50, 45 / 200, 10 / 50]), 1 / 16))
    s = r.summary()
    assert list(s.columns) == ["query", "size", "matched", "rows", "explained", "unexplained"]
    assert list(s["query"]) == ["q0", "q1", "q2"] and list(s["rows"]) == [2, 0, 1] and list(s["explained"]) == [50, 0, 10]
    assert list(s["matched"]) == [60, 0, 10] and list(s["unexplained"]) == [10, 0, 0] and list(s["size"]) == [100, 0, 40]
    # an empty db genome has no f_match; no rows: empty frames with the same columns
    from pyani_amd import screen
    odd = r._replace(db=np.array([2, 0, 1], np.int32))
    assert np.isnan(odd.frame()["f_match"].to_numpy()[0]) and np.isnan(odd.frame()["identity"].to_numpy()[0])
    z32, zu = np.zeros(0, np.int32), np.zeros(0, np.uint32)
    empty = screen.GatherResult(["q"], ["d"], screen.GatherOptions(16, 16, 1), np.array([5], np.uint32), np.array([5], np.uint32), z32, z32, zu, zu, np.array([0], np.uint32))
    assert len(empty.frame()) == 0 and list(empty.frame().columns) == list(f.columns) and list(empty.summary()["rows"]) == [0]


def test_the_calls_are_declared_bound_and_exported():
    from pyani_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    build.build_gpu()
    lib = _lib.load()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "pgscr_gather.inc" in (ROOT / "pyani_amd" / "csrc" / "pg_screen.hip").read_text()
    assert len(_lib.SIGNATURES["pg_screen_gather"][1]) == 5 and len(_lib.SIGNATURES["pg_screen_gather_read"][1]) == 5


class _StubLib:
    """Records the calls; every query `i` of a count has size 100 + i, matched 10 and one row (db 1, unique 5, total 7)."""

    def __init__(self, fail_at=None):
        self.calls, self.fail_at, self.q = [], fail_at, 0

    def _arr(self, addr, n, dtype):
        import ctypes
        return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,))

    def pg_screen_search_index(self, *a):
        return 0

    def pg_screen_gather_count(self, h, ids, q, sizes):
        self.calls.append(("gather_count", q))
        if self.fail_at == len([c for c in self.calls if c[0] == "gather_count"]):
            return -5
        self.q = q
        self._arr(sizes, q, np.uint32)[:] = 100 + np.arange(q)
        return 0

    def pg_screen_search_count(self, h, ids, q, sizes):
        self.calls.append(("search_count", q))
        return 0

    def pg_screen_gather_matched(self, h, out):
        self._arr(out, self.q, np.uint32)[:] = 10
        return 0

    def pg_screen_gather(self, h, need, q, max_ranks, n_rows):
        self.calls.append(("gather", q, max_ranks, self._arr(need, q, np.uint32).tolist()))
        n_rows._obj.value = q
        return 0

    def pg_screen_gather_read(self, h, qo, do, uo, to):
        self._arr(qo, self.q, np.int32)[:] = np.arange(self.q)
        self._arr(do, self.q, np.int32)[:] = 1
        self._arr(uo, self.q, np.uint32)[:] = 5
        self._arr(to, self.q, np.uint32)[:] = 7
        return 0

    def pg_last_error(self, h):
        return b"stub"


def _stub_engine(lib, band_rows):
    from pyani_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._h = lib, None
    e.screen_search_index([0, 1, 2], 16, 16, labels=["a", "b", "c"])
    e._band_rows = band_rows
    return e


def test_engine_screen_gather_works_in_chunks_and_releases():
    from pyani_amd import _lib, screen
    lib = _StubLib()
    e = _stub_engine(lib, 3)
    r = e.screen_gather(list(range(10, 17)), screen.GatherOptions(16, 16, 4, 0.05, 9), query_labels=[f"q{i}" for i in range(7)])
    assert [c for c in lib.calls if c[0] != "gather"] == [("gather_count", 3), ("gather_count", 3), ("gather_count", 1), ("search_count", 0)]
    assert [c[1:3] for c in lib.calls if c[0] == "gather"] == [(3, 9), (3, 9), (1, 9)]
    assert [c[3] for c in lib.calls if c[0] == "gather"] == [[5, 6, 6], [5, 6, 6], [5]]      # max(4, ceil(0.05 (100 + i))), per chunk
    assert r.query.tolist() == list(range(7)) and r.db.tolist() == [1] * 7 and r.unique.tolist() == [5] * 7 and r.total.tolist() == [7] * 7
    assert r.query_sizes.tolist() == [100, 101, 102, 100, 101, 102, 100] and r.matched.tolist() == [10] * 7 and r.db_labels == ["a", "b", "c"]
    assert list(r.frame()["query"]) == [f"q{i}" for i in range(7)] and list(r.summary()["unexplained"]) == [5] * 7
    # an error in the second chunk: the kept entries of the first are released all the same, and the error is the count's
    lib = _StubLib(fail_at=2)
    e = _stub_engine(lib, 3)
    with pytest.raises(_lib.PyaniGpuError) as err:
        e.screen_gather(list(range(7)), screen.GatherOptions(16, 16, 4))
    assert err.value.code == _lib.PG_E_NOMEM and lib.calls[-1] == ("search_count", 0) and [c[0] for c in lib.calls].count("gather_count") == 2
    # refusals before any call
    lib = _StubLib()
    e = _stub_engine(lib, 3)
    with pytest.raises(ValueError, match="kmer 16 and scale 16"):
        e.screen_gather([0], screen.GatherOptions(12, 16, 4))
    with pytest.raises(ValueError, match="GatherOptions"):
        e.screen_gather([0], 0.9)
    with pytest.raises(ValueError, match="same length"):
        e.screen_gather([0, 1], screen.GatherOptions(16, 16, 4), query_labels=["x"])
    assert lib.calls == []
    e._search = None
    with pytest.raises(ValueError, match="no search index"):
        e.screen_gather([0], screen.GatherOptions(16, 16, 4))


def test_driver_refusals_come_before_any_work(tmp_path):
    from pyani_amd.subcmd_gather import run_screen_gather

    class NoEngine:      # any use would raise AttributeError, not ValueError
        pass
    missing = tmp_path / "does_not_exist"
    with pytest.raises(ValueError, match="min_unique"):
        run_screen_gather(missing, missing, engine=NoEngine())
    with pytest.raises(ValueError, match="output directory"):
        run_screen_gather(missing, missing, min_unique=5, write_output=True, engine=NoEngine())
    with pytest.raises(ValueError, match="exact"):
        run_screen_gather(missing, missing, min_unique=5, exact="anib", engine=NoEngine())
    with pytest.raises(ValueError, match="single engine"):
        run_screen_gather(missing, missing, min_unique=5, devices=[0, 1])
    with pytest.raises(ValueError, match="single engine"):
        run_screen_gather(missing, missing, min_unique=5, workers=2)
    with pytest.raises(ValueError, match="8 ... 16"):
        run_screen_gather(missing, missing, min_unique=5, kmer=17, engine=NoEngine())
    with pytest.raises(ValueError, match="max_ranks"):
        run_screen_gather(missing, missing, min_unique=5, max_ranks=0, engine=NoEngine())
