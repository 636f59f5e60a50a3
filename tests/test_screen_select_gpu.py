"""GPU (through the C ABI): the screen's selection on the device (pg_screen_hold / _load / _select / _select_read / _fetch / _release,
pyani_amd/csrc/pg_screen.hip) against the numpy statement of its rule (tests/screen_select_cases.rule; proved equal to
ScreenResult.candidate_pairs by tests/test_screen_select_cpu.py).  Everything is an integer and must be EQUAL: the same triples in the
same order."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

U32_MAX = 2 ** 32 - 1
# the wave (64), the workgroup (256), a wave's task (512 cells) and, at 2049 (2049 x 5 tasks), the grid: each from below, at and above
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1100, 2049)


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


def _same(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.int32, np.uint32), "abs"):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def crafted(n):
    """(name, shared uint32[n, n], need uint32[n]) of the cases every size is held to."""
    rng = np.random.default_rng(1000 + n)
    idx = np.arange(n)
    # any content: asymmetric, the diagonal 2^32 - 1, about a tenth kept
    m = rng.integers(0, 1000, (n, n)).astype(np.uint32)
    m[idx, idx] = U32_MAX
    yield "random, asymmetric", m, rng.integers(850, 1100, n).astype(np.uint32)
    # everything: n (n - 1) triples in row-major order
    yield "everything kept", m, np.zeros(n, dtype=np.uint32)
    # nothing, whatever the diagonal holds
    yield "nothing kept", m, np.full(n, 1000, dtype=np.uint32)
    yield "nothing kept, the largest threshold", m, np.full(n, U32_MAX, dtype=np.uint32)
    if n >= 2:
        one = np.zeros((n, n), dtype=np.uint32)
        one[idx, idx] = U32_MAX
        one[n - 1, n - 2] = 7
        yield "one pair, the last off-diagonal cell", one, np.full(n, 7, dtype=np.uint32)
        rows = np.zeros((n, n), dtype=np.uint32)
        rows[(idx % 3 == 0) | (idx == n - 1)] = 5      # full rows with empty rows between them
        yield "empty rows between full rows", rows, np.full(n, 5, dtype=np.uint32)
        # cells at and one below BOTH thresholds of their pair, need[a] != need[b] for nearly every pair
        need = (10 + 2 * rng.permutation(n)).astype(np.uint32)
        lo, hi = np.minimum.outer(need, need).astype(np.int64), np.maximum.outer(need, need).astype(np.int64)
        pick = rng.integers(0, 4, (n, n))
        edge = np.choose(pick, [lo - 1, lo, hi - 1, hi]).astype(np.uint32)
        yield "at and below either side's threshold", edge, need


@pytest.mark.parametrize("n", SIZES)
def test_select_equals_the_rule(eng, n):
    seen = 0
    for name, shared, need in crafted(n):
        eng.screen_load(shared)
        got = eng.screen_select(need)
        want = ssc.rule(shared, need)
        _same(got, want, (n, name))
        if name == "everything kept":
            assert len(got[0]) == n * (n - 1)
            assert (got[0] == np.repeat(np.arange(n), n - 1)).all() and (got[1] == np.array([b for a in range(n) for b in range(n) if a != b], dtype=np.int64)).all()
        if name.startswith("nothing"):
            assert len(got[0]) == 0
        if name.startswith("one pair"):
            assert [x.tolist() for x in got] == [[n - 1], [n - 2], [7]]
        if name.startswith("at and below") and n >= 63:      # (four kinds of cell drawn at random: both outcomes occur once there are enough)
            assert 0 < len(got[0]) < n * (n - 1)
        seen += 1
    assert seen == (7 if n >= 2 else 4)
    eng.screen_release()


def test_two_selections_on_one_resident_matrix(eng):
    sizes, shared = ssc.random_symmetric(11, 300)
    eng.screen_load(shared)
    from pyani_amd.screen import identity_thresholds
    lists = []
    for t in (0.9, 0.5, 0.999, 0.0):      # a longer list after a shorter one and the other way round
        need = identity_thresholds(sizes, 16, t, 2)
        got = eng.screen_select(need)
        _same(got, ssc.rule(shared, need), t)
        lists.append(len(got[0]))
    assert lists[3] == 300 * 299 and 0 < lists[2] < lists[0] < lists[1] < lists[3]
    assert (eng.screen_fetch() == shared).all()      # the selections left the matrix alone
    eng.screen_release()


@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("family", 12, 16), ("edges", *scr.EDGES_PARAMS)])
def test_hold_fetch_and_candidates_equal_the_matrix_path(case, k, scale):
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in scr.CASES[case]()]
        n = len(ids)
        want_sizes, want_shared = e.screen_matrix(ids, kmer=k, scale=scale)
        assert (want_sizes == scr.expected(case, k, scale)[0]).all() and (want_shared == scr.expected(case, k, scale)[1]).all()
        last = e.screen_last()
        sizes = e.screen_hold(ids, kmer=k, scale=scale)
        assert sizes.dtype == np.uint32 and (sizes == want_sizes).all() and (e.screen_fetch() == want_shared).all()
        assert {x: v for x, v in e.screen_last().items() if not x.endswith("_ms")} == {x: v for x, v in last.items() if not x.endswith("_ms")}
        # parts, and a budget that cuts the keys into slices: the held matrix is the matrix call's
        parts = []
        for p in range(3):
            s = e.screen_hold(ids, kmer=k, scale=scale, part=p, n_parts=3)
            parts.append((s, e.screen_fetch()))
            m = e.screen_matrix(ids, kmer=k, scale=scale, part=p, n_parts=3)
            assert (m[0] == s).all() and (m[1] == parts[-1][1]).all()
        assert (sum(p[0] for p in parts) == want_sizes).all() and (sum(p[1] for p in parts) == want_shared).all()
        try:
            e.screen_set_budget(max(last["keys"] // 3, 1))
            sizes = e.screen_hold(ids, kmer=k, scale=scale)
            assert e.screen_last()["slices"] >= 3 and (sizes == want_sizes).all() and (e.screen_fetch() == want_shared).all()
        finally:
            e.screen_set_budget(0)
        # screen_candidates == candidate_pairs of the ScreenResult, in content and in order; nothing stays resident
        labels = [f"g{i}" for i in range(n)]
        res = screen.screen_genomes(e, ids, labels, kmer=k, scale=scale)
        lengths = set()
        for t in ssc.THRESHOLDS:
            for ms in (1, 2):
                sp = e.screen_candidates(ids, screen.ScreenOptions(t, k, scale, ms), labels=labels)
                assert sp.pairs() == res.candidate_pairs(t, ms), (t, ms)
                assert sp.labels == labels and (sp.sizes == want_sizes).all() and (sp.shared == want_shared[sp.a, sp.b]).all()
                ident = res._identity(ms)[sp.a, sp.b]
                np.testing.assert_allclose(sp.identity(), ident, rtol=4 * np.finfo(np.float64).eps, atol=0.0)      # the same expression on other array shapes
                lengths.add(len(sp.a))
                with pytest.raises(Exception):
                    e.screen_fetch()
        assert 0 in lengths or min(lengths) < n * (n - 1)
        assert max(lengths) == n * (n - 1) and len(lengths) >= 3
        assert e.screen_candidates(ids, 0.8, labels=labels).options == screen.ScreenOptions(0.8)      # a bare float
        assert e.screen_candidates([], 0.8).pairs() == []
        # the genome store going takes the matrix with it
        e.screen_hold(ids, kmer=k, scale=scale)
        e.clear_genomes()
        with pytest.raises(Exception):
            e.screen_fetch()


def test_refusals_leave_the_engine_usable(eng):
    from pyani_amd import _lib
    sizes, shared = ssc.random_symmetric(12, 70)
    need = np.full(70, 3, dtype=np.uint32)
    want = ssc.rule(shared, need)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    eng.screen_release()
    eng.screen_release()      # nothing resident: still fine
    refused(lambda: eng.screen_select(need), "no resident matrix")
    refused(lambda: eng.screen_fetch(), "no resident matrix")
    eng.screen_load(shared)
    _same(eng.screen_select(need), want, "after select without a matrix")
    refused(lambda: eng.screen_select(need[:69]), "not 69")
    refused(lambda: eng.screen_select(np.zeros(71, dtype=np.uint32)), "not 71")
    refused(lambda: eng.screen_select(np.zeros(8193, dtype=np.uint32)), "not 8193")
    _same(eng.screen_select(need), want, "after a size mismatch")
    refused(lambda: eng.screen_load(np.zeros((8193, 8193), dtype=np.uint32)), "8192")      # (refused before the matrix is read)
    refused(lambda: eng.screen_hold(list(range(8193))), "8192")
    with pytest.raises(ValueError):
        eng.screen_load(np.zeros((3, 4), dtype=np.uint32))
    _same(eng.screen_select(need), want, "after refused loads")      # a call refused for its arguments leaves the resident matrix alone
    eng.screen_release()
    refused(lambda: eng.screen_select(need), "no resident matrix")      # release, then select
    eng.screen_load(shared)
    _same(eng.screen_select(need), want, "after a release")
    eng.screen_release()
