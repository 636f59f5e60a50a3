"""CPU: the host side of the gather's abundances — the statement of tests/screen_abund_cases.py against a brute-force
recount over a random tiny incidence with multiset counts; GatherOptions.abundance; the abundance columns of GatherResult.frame() and
.summary() from given integers, and both frames unchanged without them; the five calls declared, bound and exported; Engine.screen_gather
carrying the arrays through the chunks on a stub library.  No device."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import screen_abund_cases as sac
from tests import screen_gather_cases as sgc

ROOT = Path(__file__).resolve().parent.parent
CALLS = {"pg_screen_gather_count_abund": 5, "pg_screen_gather_abund": 2, "pg_screen_gather_abund_read": 6, "pg_screen_gather_abund_matched": 2,
         "pg_screen_gather_abund_last": 3}      # name -> arguments
PLAIN_ROWS = ["query", "rank", "db", "unique", "total", "f_unique_query", "f_unique_cumulative", "f_match", "identity"]
PLAIN_SUMMARY = ["query", "size", "matched", "rows", "explained", "unexplained"]
ABUND_ROWS = ["average_abund", "median_abund", "std_abund", "f_unique_weighted", "f_weighted_cumulative"]
ABUND_SUMMARY = ["weight", "matched_weight", "explained_weight", "unexplained_weight"]


@pytest.fixture(autouse=True, scope="module")
def _the_feature_is_there():
    """This file is about the abundances: without them in the package none of it says anything."""
    from pyani_amd import screen
    assert "abundance" in screen.GatherOptions._fields and hasattr(screen, "abundance_columns")


def _brute(query_lists, db_sets, need, max_ranks):
    """Another route to the statistics: the query as a LIST of occurrences; every occurrence is given to the first winner (in the order
    of the rounds) that holds its k-mer, and a row's multiplicities are recounted from the occurrences it was given."""
    out, unattributed = [], 0
    for i, occurrences in enumerate(query_lists):
        rest, winners = set(occurrences), []
        while len(winners) < max_ranks:
            left = [len(rest & set(s)) for s in db_sets]
            w = left.index(max(left)) if left else 0
            if not left or left[w] < need[i]:
                break
            winners.append(w)
            rest -= set(db_sets[w])
        given = [[] for _ in winners]
        for x in occurrences:
            for t, w in enumerate(winners):
                if x in db_sets[w]:
                    given[t].append(x)
                    break
        union = set().union(*[set(s) for s in db_sets]) if db_sets else set()
        unattributed += len({x for x in occurrences if x in union and not any(x in db_sets[w] for w in winners)})
        for t, w in enumerate(winners):
            a = sorted(given[t].count(x) for x in set(given[t]))
            out.append((i, w, len(a), sum(a), sum(v * v for v in a), a[(len(a) - 1) // 2] + a[len(a) // 2], a[0], a[-1]))
    return out, unattributed


@pytest.mark.parametrize("seed", range(6))
def test_the_statement_is_the_brute_force_recount(seed):
    rng = np.random.default_rng(100 + seed)
    n, q, universe = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(4, 40))
    db = [set(rng.choice(universe, size=int(rng.integers(0, universe)), replace=False).tolist()) for _ in range(n)]
    if n >= 3:
        db[2] = set(db[0])      # a tie of whole genomes
    queries = [rng.integers(0, universe + 5, size=int(rng.integers(0, 4 * universe))).tolist() for _ in range(q)]      # with repeats
    counts = [{x: lst.count(x) for x in set(lst)} for lst in queries]
    for need, max_ranks in ((1, 65536), (3, 65536), (1, 2)):
        want = sac.abundance_sets(counts, db, [need] * q, max_ranks)
        g = want.gathered
        rows, unattributed = _brute(queries, db, [need] * q, max_ranks)
        assert list(zip(g.query.tolist(), g.db.tolist(), g.unique.tolist(), want.sum, want.sumsq, want.median2, want.min, want.max)) == rows, (seed, need, max_ranks)
        assert want.unattributed == unattributed
        union = set().union(*db)
        assert want.weight == [len(lst) for lst in queries]
        assert want.matched_weight == [sum(1 for x in lst if x in union) for lst in queries]
        explained = sac.summary_columns(want)
        assert all(u >= 0 for u in explained["unexplained_weight"]) and sum(explained["explained_weight"]) == sum(want.sum)
        for i in range(q):      # the unexplained weight is the weight of the matched k-mers that belong to no row
            winners = g.db[g.query == i].tolist()
            stay = sum(1 for x in queries[i] if x in union and not any(x in db[w] for w in winners))
            assert explained["unexplained_weight"][i] == stay


def test_the_median_and_the_two_words():
    want = sac.abundance_sets([{1: 5, 2: 1, 3: 2, 4: 9, 7: 4}], [{1, 2, 3, 4}, {7, 4}], [1], 65536)
    assert want.gathered.db.tolist() == [0, 1] and want.gathered.unique.tolist() == [4, 1]
    assert want.median2 == [2 + 5, 4 + 4] and want.min == [1, 4] and want.max == [9, 4] and want.sum == [17, 4] and want.sumsq == [111, 16]
    assert want.weight == [21] and want.matched_weight == [21] and want.unattributed == 0 and want.holders == 6
    from pyani_amd import screen
    big = (1 << 32) - 1
    words = screen.sumsq_words(np.array([[5, 0], [(3 * big * big) & ((1 << 64) - 1), (3 * big * big) >> 64]], dtype=np.uint64))
    assert words.dtype == object and words.tolist() == [5, 3 * big * big] and all(type(x) is int for x in words)


def test_gather_options_abundance():
    from pyani_amd import screen
    assert screen.GatherOptions(16, 256, 50).abundance is False
    assert screen.GatherOptions(16, 256, 50, 0.1, 7) == screen.GatherOptions(16, 256, 50, 0.1, 7, False)      # the first five positionally, as before
    o = screen.check_gather_options(screen.GatherOptions(16, 256, 50, abundance=True))
    assert o == screen.GatherOptions(16, 256, 50, 0.0, 65536, True) and o.abundance is True
    assert screen.check_gather_options(screen.GatherOptions(16, 256, 50, 0.0, 9, np.bool_(True))).abundance is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="abundance"):
            screen.check_gather_options(screen.GatherOptions(16, 256, 50, 0.0, 9, bad))


def _result(abundance):
    from pyani_amd import screen
    big = (1 << 32) - 1
    plain = (["q0", "q1", "q2"], ["d0", "d1", "d2"], screen.GatherOptions(16, 16, 1, abundance=abundance), np.array([100, 0, 40], np.uint32),
             np.array([200, 50, 0], np.uint32), np.array([0, 0, 2], np.int32), np.array([1, 0, 1], np.int32), np.array([30, 20, 3], np.uint32),
             np.array([30, 45, 10], np.uint32), np.array([60, 0, 10], np.uint32))
    if not abundance:
        return screen.GatherResult(*plain), None
    ints = {"weight": [7001, 0, 3 * big + 11], "matched_weight": [4000, 0, 3 * big + 5], "sum": [901, 77, 3 * big],
            "sumsq": [40_001, 1_301, 3 * big * big], "median2": [59, 8, 2 * big], "min": [1, 2, big], "max": [400, 30, big]}
    sumsq = np.empty(3, dtype=object)
    sumsq[:] = ints["sumsq"]
    return screen.GatherResult(*plain, np.array(ints["weight"], np.uint64), np.array(ints["matched_weight"], np.uint64), np.array(ints["sum"], np.uint64), sumsq,
                               np.array(ints["median2"], np.uint64), np.array(ints["min"], np.uint32), np.array(ints["max"], np.uint32)), ints


def test_the_columns_are_the_formulas_bit_for_bit():
    r, v = _result(True)
    f, s = r.frame(), r.summary()
    assert list(f.columns) == PLAIN_ROWS + ABUND_ROWS and list(s.columns) == PLAIN_SUMMARY + ABUND_SUMMARY
    m, q = [30, 20, 3], [0, 0, 2]
    assert f["average_abund"].tolist() == [v["sum"][j] / m[j] for j in range(3)]
    assert f["median_abund"].tolist() == [v["median2"][j] / 2 for j in range(3)]
    assert f["std_abund"].tolist() == [math.sqrt((m[j] * v["sumsq"][j] - v["sum"][j] ** 2) / m[j] ** 2) for j in range(3)]
    assert f["f_unique_weighted"].tolist() == [v["sum"][j] / v["weight"][q[j]] for j in range(3)]
    assert f["f_weighted_cumulative"].tolist() == [901 / 7001, (901 + 77) / 7001, v["sum"][2] / v["weight"][2]]      # starts again with every query
    # the division of two ints is the correctly rounded quotient: the same as the exact fraction rounded once
    assert f["average_abund"].tolist() == [float(Fraction(v["sum"][j], m[j])) for j in range(3)]
    assert f["std_abund"].tolist()[2] == 0.0 and f["median_abund"].tolist()[2] == float((1 << 32) - 1)      # three equal values beyond 2^31
    assert s["weight"].tolist() == v["weight"] and s["matched_weight"].tolist() == v["matched_weight"]
    assert s["explained_weight"].tolist() == [901 + 77, 0, v["sum"][2]] and s["unexplained_weight"].tolist() == [4000 - 978, 0, 5]
    assert s["weight"].dtype == np.uint64 and s["unexplained_weight"].dtype == np.uint64
    # the statement's own columns, from the same integers
    want = sac.Abundances(sgc.Gathered(r.query, r.db, r.unique, r.total, None, None, r.matched, 0, 0, 0), v["weight"], v["matched_weight"], v["sum"], v["sumsq"],
                          v["median2"], v["min"], v["max"], 0, 0)
    for name, column in sac.columns(want).items():
        assert f[name].tolist() == column, name
    for name, column in sac.summary_columns(want).items():
        assert s[name].tolist() == column, name


def test_both_frames_are_unchanged_without_the_fields():
    plain, _ = _result(False)
    with_fields, _ = _result(True)
    assert plain.query_weight is None and plain.sum_abund is None and not plain.has_abundance() and with_fields.has_abundance()
    f, s = plain.frame(), plain.summary()
    assert list(f.columns) == PLAIN_ROWS and list(s.columns) == PLAIN_SUMMARY
    assert f.equals(with_fields.frame()[PLAIN_ROWS]) and s.equals(with_fields.summary()[PLAIN_SUMMARY])
    assert np.array_equal(f["f_unique_cumulative"].to_numpy(), [30 / 100, 50 / 100, 3 / 40]) and list(s["explained"]) == [50, 0, 3]
    # no rows: empty columns of the right names
    from pyani_amd import screen
    z32, zu, z64 = np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    empty = screen.GatherResult(["q"], ["d"], screen.GatherOptions(16, 16, 1, abundance=True), np.array([5], np.uint32), np.array([5], np.uint32), z32, z32, zu, zu,
                                np.array([0], np.uint32), np.array([9], np.uint64), np.array([0], np.uint64), z64, np.zeros(0, object), z64, zu, zu)
    assert len(empty.frame()) == 0 and list(empty.frame().columns) == PLAIN_ROWS + ABUND_ROWS
    assert empty.summary()["weight"].tolist() == [9] and empty.summary()["unexplained_weight"].tolist() == [0]


def test_the_calls_are_declared_bound_and_exported():
    from pyani_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    build.build_gpu()
    lib = _lib.load()
    for name, n_args in CALLS.items():
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert declared and len(declared.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name), name
    assert "pgscr_abund.inc" in (ROOT / "pyani_amd" / "csrc" / "pg_screen.hip").read_text()


class _StubLib:
    """Every query i of a count has size 100 + i, weight 1000 + i, matched 10, matched weight 50 and one row (db 1, unique 5, total 7)
    with the statistics sum 20 + i, sumsq (400 + i, i), median2 8, min 2, max 9."""

    def __init__(self):
        self.calls, self.q = [], 0

    def _arr(self, addr, n, dtype):
        import ctypes
        return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,))

    def pg_screen_search_index(self, *a):
        return 0

    def pg_screen_gather_count_abund(self, h, ids, q, sizes, weight):
        self.calls.append(("count_abund", q))
        self.q = q
        self._arr(sizes, q, np.uint32)[:] = 100 + np.arange(q)
        self._arr(weight, q, np.uint64)[:] = 1000 + np.arange(q)
        return 0

    def pg_screen_gather_count(self, h, ids, q, sizes):
        self.calls.append(("count", q))
        self.q = q
        self._arr(sizes, q, np.uint32)[:] = 100 + np.arange(q)
        return 0

    def pg_screen_search_count(self, h, ids, q, sizes):
        self.calls.append(("search_count", q))
        return 0

    def pg_screen_gather_matched(self, h, out):
        self._arr(out, self.q, np.uint32)[:] = 10
        return 0

    def pg_screen_gather_abund_matched(self, h, out):
        self.calls.append(("abund_matched",))
        self._arr(out, self.q, np.uint64)[:] = 50
        return 0

    def pg_screen_gather(self, h, need, q, max_ranks, n_rows):
        self.calls.append(("gather", q))
        n_rows._obj.value = q
        return 0

    def pg_screen_gather_read(self, h, qo, do, uo, to):
        self._arr(qo, self.q, np.int32)[:] = np.arange(self.q)
        self._arr(do, self.q, np.int32)[:] = 1
        self._arr(uo, self.q, np.uint32)[:] = 5
        self._arr(to, self.q, np.uint32)[:] = 7
        return 0

    def pg_screen_gather_abund(self, h, n_rows):
        self.calls.append(("abund", self.q))
        n_rows._obj.value = self.q
        return 0

    def pg_screen_gather_abund_read(self, h, so, sqo, mo, lo, ho):
        self._arr(so, self.q, np.uint64)[:] = 20 + np.arange(self.q)
        words = self._arr(sqo, 2 * self.q, np.uint64)
        words[0::2] = 400 + np.arange(self.q)
        words[1::2] = np.arange(self.q)
        self._arr(mo, self.q, np.uint64)[:] = 8
        self._arr(lo, self.q, np.uint32)[:] = 2
        self._arr(ho, self.q, np.uint32)[:] = 9
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


def test_engine_screen_gather_carries_the_abundances_through_the_chunks():
    from pyani_amd import screen
    lib = _StubLib()
    e = _stub_engine(lib, 3)
    r = e.screen_gather(list(range(10, 17)), screen.GatherOptions(16, 16, 4, abundance=True))
    assert [c[0] for c in lib.calls] == ["count_abund", "abund_matched", "gather", "abund"] * 3 + ["search_count"]      # the concluding empty count stays
    assert [c[1] for c in lib.calls if c[0] == "count_abund"] == [3, 3, 1]
    assert r.query.tolist() == list(range(7)) and r.has_abundance()
    assert r.query_weight.dtype == np.uint64 and r.query_weight.tolist() == [1000, 1001, 1002, 1000, 1001, 1002, 1000] and r.matched_weight.tolist() == [50] * 7
    assert r.sum_abund.tolist() == [20, 21, 22, 20, 21, 22, 20] and r.median2_abund.tolist() == [8] * 7 and r.min_abund.tolist() == [2] * 7 and r.max_abund.tolist() == [9] * 7
    assert r.sumsq_abund.dtype == object and r.sumsq_abund.tolist() == [400, 401 + (1 << 64), 402 + (2 << 64), 400, 401 + (1 << 64), 402 + (2 << 64), 400]
    assert r.summary()["unexplained_weight"].tolist() == [30, 29, 28, 30, 29, 28, 30]
    # with the option off: the plain calls, the plain fields
    lib = _StubLib()
    e = _stub_engine(lib, 3)
    r = e.screen_gather(list(range(4)), screen.GatherOptions(16, 16, 4))
    assert [c[0] for c in lib.calls] == ["count", "gather", "count", "gather", "search_count"] and not r.has_abundance() and len(r) == 17
    assert list(r.frame().columns) == PLAIN_ROWS


def test_the_driver_takes_the_option(tmp_path):
    import inspect
    from pyani_amd.subcmd_gather import run_screen_gather
    assert inspect.signature(run_screen_gather).parameters["abundance"].default is False

    class NoEngine:
        pass
    with pytest.raises(ValueError, match="abundance"):
        run_screen_gather(tmp_path, tmp_path, min_unique=5, abundance=1, engine=NoEngine())
