"""pg_anib_rows_batch / Engine.anib_rows_batch: the tables of many ordered pairs from one call, packed on the device (an exclusive
scan over the per-fragment row counts + a pack pass, pga_frag.inc), in the caller's pair order.

The bar everywhere is EQUALITY, field for field, with what the single-pair calls give (anib_pair_rows: the padded scratch of one
pair compacted on the host; anib_pairs: the pair tuple), and where stated with the CPU statement (oracle/anib_cpu.cpp)."""
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))
import anib_cpu  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("frag", "length", "mismatch", "gaps", "nident", "qlen", "qstart", "qend", "sstart", "send", "srec", "score")
DEFAULT_BUDGET = (131072, 512 << 20)      # pg_internal.h: anim_batch_pairs, anim_batch_matches


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _rows(a):
    return [tuple(int(r[k]) for k in FIELDS) for r in a]


def _check_offsets(off, rows, n):
    off = np.asarray(off, dtype=np.int64)
    assert len(off) == n + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(rows)


def _assert_equals_single_calls(eng, qs, ss, res, off, rows, fragsize, singles=None):
    """Every pair of the batch against anib_pair_rows / anib_pairs of that pair alone (cached per (q, s) in `singles`)."""
    singles = {} if singles is None else singles
    _check_offsets(off, rows, len(qs))
    for i, (q, s) in enumerate(zip(qs, ss)):
        if (q, s) not in singles:
            singles[(q, s)] = (_rows(eng.anib_pair_rows(q, s, fragsize)), tuple(eng.anib_pairs([q], [s], fragsize)[0]))
        want_rows, want_rec = singles[(q, s)]
        assert _rows(rows[int(off[i]):int(off[i + 1])]) == want_rows, (i, q, s)
        assert tuple(res[i]) == want_rec, (i, q, s)
    return singles


def test_batch_equals_single_pair_calls_in_caller_order(eng):
    """Six related genomes of ~25 kb at fragsize 500 plus the tiny / all-N / empty genomes: 38 ordered pairs in a shuffled order
    (not grouped by subject), one pair twice, one genome against itself."""
    from pyani_amd import synth
    eng.clear_genomes()
    g = [eng.add_genome(*synth.genome(20250302, 6, k, 25_000)) for k in range(6)]
    tiny = eng.add_genome(np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8), np.array([0, 14], dtype=np.uint64))
    alln = eng.add_genome(np.frombuffer(b"N" * 3000, dtype=np.uint8), np.array([0, 3000], dtype=np.uint64))
    empty = eng.add_genome(np.zeros(0, dtype=np.uint8), np.array([0, 0], dtype=np.uint64))
    pairs = [(a, b) for a in g for b in g if a != b]
    pairs += [(g[0], tiny), (tiny, g[0]), (g[1], alln), (alln, g[1]), (g[2], empty), (empty, g[2]), (g[0], g[0]), (g[1], g[2])]
    order = np.random.RandomState(11).permutation(len(pairs))
    pairs = [pairs[k] for k in order]
    qs, ss = [p[0] for p in pairs], [p[1] for p in pairs]
    assert len(pairs) == 38 and pairs.count((g[1], g[2])) == 2
    assert sum(1 for a, b in zip(ss, ss[1:]) if a != b) > 20      # the subjects alternate: not grouped
    res, off, rows = eng.anib_rows_batch(qs, ss, fragsize=500)
    _assert_equals_single_calls(eng, qs, ss, res, off, rows, 500)
    counts = np.diff(np.asarray(off, dtype=np.int64))
    odd = {tiny, alln, empty}
    for i, (q, s) in enumerate(pairs):
        if q in odd or s in odd:
            assert counts[i] == 0 and int(res[i]["status"]) == 0, (i, q, s)
    self_at = pairs.index((g[0], g[0]))
    assert counts[self_at] >= int(res[self_at]["n_kept"]) > 40
    assert counts.sum() > 1000


def test_chunk_and_worker_boundaries_do_not_show(eng):
    """72 ordered pairs (both workers run, n >= 64) under a budget of 16 pairs in flight: several launches per worker.  The result
    equals the default budget's and the single-pair calls'."""
    from pyani_amd import synth
    eng.clear_genomes()
    g = [eng.add_genome(*synth.genome(77, 9, k, 6_000)) for k in range(9)]
    pairs = [(a, b) for a in g for b in g if a != b]
    order = np.random.RandomState(5).permutation(len(pairs))
    qs, ss = [pairs[k][0] for k in order], [pairs[k][1] for k in order]
    assert len(qs) == 72
    want = eng.anib_rows_batch(qs, ss)
    try:
        eng.anim_set_batch_budget(16, DEFAULT_BUDGET[1])
        got = eng.anib_rows_batch(qs, ss)
    finally:
        eng.anim_set_batch_budget(*DEFAULT_BUDGET)
    assert (np.asarray(got[1]) == np.asarray(want[1])).all() and _rows(got[2]) == _rows(want[2])
    assert [tuple(r) for r in got[0]] == [tuple(r) for r in want[0]]
    _assert_equals_single_calls(eng, qs, ss, *got, 1020)
    assert int(got[1][-1]) > 200


def test_rows_are_packed_after_the_word_tier(eng):
    """A pair diverged enough that the 16-mer seeds leave some fragments without a reportable hit (0 < n_kept < n_frags: the word
    tier runs and rewrites rows): batch rows == anib_pair_rows == the CPU statement's rows."""
    from pyani_amd import synth
    eng.clear_genomes()
    n, L, seed = 6, 150_000, 20250302      # the divergence levels of test_anib_gpu.test_rows_equal_cpu_statement_on_synthetic_pairs
    data = [synth.genome(seed, n, k, L) for k in range(n)]
    ids = [eng.add_genome(*d) for d in data]
    recs = eng.anib_pairs([ids[0]] * (n - 1), ids[1:])
    tier = [k for k in range(1, n) if 0 < int(recs[k - 1]["n_kept"]) < int(recs[k - 1]["n_frags"])]
    assert tier, [(int(r["n_kept"]), int(r["n_frags"])) for r in recs]      # otherwise this test shows nothing
    b = tier[-1]                                                               # the most diverged of them
    res, off, rows = eng.anib_rows_batch([ids[0], ids[b]], [ids[b], ids[0]])
    assert 0 < int(res[0]["n_kept"]) < int(res[0]["n_frags"])
    _assert_equals_single_calls(eng, [ids[0], ids[b]], [ids[b], ids[0]], res, off, rows, 1020)
    want = _rows(anib_cpu.anib_cpu_pair(data[0], data[b]))
    assert _rows(rows[:int(off[1])]) == want and len(want) > 50


def test_tiny_fragment_size_thousands_of_empty_slots(eng):
    """fragsize = 30 on a 60 kb genome against itself and against another: thousands of (pair, fragment) slots, almost all
    without a row — the scan's offsets mostly repeat."""
    from pyani_amd import synth
    eng.clear_genomes()
    a = eng.add_genome(*synth.genome(5, 4, 0, 60_000))
    b = eng.add_genome(*synth.genome(5, 4, 1, 60_000))
    qs, ss = [a, a, b], [a, b, a]
    res, off, rows = eng.anib_rows_batch(qs, ss, fragsize=30)
    assert int(res[0]["n_frags"]) >= 2000 and (res["status"] == 0).all()
    _assert_equals_single_calls(eng, qs, ss, res, off, rows, 30)
    res, off, rows = eng.anib_rows_batch(qs, ss, fragsize=333)      # (and a size that is no divisor of anything)
    _assert_equals_single_calls(eng, qs, ss, res, off, rows, 333)
    assert int(off[-1]) > 300


def test_one_real_pair_and_its_reverse(eng, genome_dir):
    """NC_014100 against NC_002696 (4 565 fragments, a two-record subject) batched with its reverse."""
    eng.clear_genomes()
    q = eng.add_fasta(genome_dir["caulobacter"]["NC_014100"])[0]
    s = eng.add_fasta(genome_dir["caulobacter"]["NC_002696"])[0]
    res, off, rows = eng.anib_rows_batch([q, s], [s, q])
    assert int(res[0]["n_frags"]) == 4565
    _assert_equals_single_calls(eng, [q, s], [s, q], res, off, rows, 1020)
    assert int(off[1]) > 2000 and int(off[2]) - int(off[1]) > 2000


def test_edge_cases():
    from pyani_amd import synth
    from pyani_amd._lib import PyaniGpuError, PG_E_ARG
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        with pytest.raises(PyaniGpuError) as err:      # nothing stored yet
            e.anib_rows_read(0)
        assert err.value.code == PG_E_ARG
        a = e.add_genome(*synth.genome(5, 4, 0, 20_000))
        b = e.add_genome(*synth.genome(5, 4, 1, 20_000))
        res, off, rows = e.anib_rows_batch([], [])
        assert len(res) == 0 and off.tolist() == [0] and len(rows) == 0
        assert len(e.anib_rows_read(0)) == 0            # an empty result is a result
        r1 = e.anib_rows_batch([a, b], [b, a])
        r2 = e.anib_rows_batch([b], [a])
        assert 0 < int(r2[1][-1]) < int(r1[1][-1])
        assert _rows(e.anib_rows_read(int(r2[1][-1]))) == _rows(r2[2]) == _rows(r1[2][int(r1[1][1]):])      # the second replaced the first
        with pytest.raises(PyaniGpuError):
            e.anib_rows_batch([a], [b], fragsize=1021)
        with pytest.raises(PyaniGpuError):
            e.anib_rows_batch([a], [99])
        with pytest.raises(ValueError):
            e.anib_rows_batch([a, b], [a])
