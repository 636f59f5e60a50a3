"""GPU: the forced re-alignment kernels (anim_postnuc_forced_kernel / _wide_kernel / _huge_kernel / _strips_kernel) on the directed
rectangles of tests/forced_cases.py, through the development entry pg_anim_forced_rects — the product's own launch function on
caller-chosen rectangles.  Every comparison is exact: error count, certified band and status against the plain-integer referee and
the host statement, and the engine counters (pg_anim_counters) against the passes the case's ladder of bands predicts for every
kernel class, so that a case that claims the group engine or the strips and does not reach them fails."""
import numpy as np
import pytest

from tests import forced_cases as fc

pytestmark = pytest.mark.gpu

KNOBS = ("PYANI_PN_WINDOW_MAX", "PYANI_PN_GROUP_MAX")


@pytest.fixture(scope="module")
def table():
    return fc.cases(), fc.expected()


def _add(eng, seq):
    return eng.add_genome(np.frombuffer(seq.encode(), dtype=np.uint8), np.array([0, len(seq)], dtype=np.uint64))


def _load(eng, cs):
    ids = {c.name: (_add(eng, c.a), _add(eng, c.b)) for c in cs}
    eng.upload()
    return ids


def _counters(eng):
    c = [int(v) for v in eng.anim_counters()]
    return c[27:31], [c[32 + 4 * k] for k in (4, 5, 6, 7)]


def _run_table(eng, ids, table, win_max=2048, group_max=8184):
    """Every case in a call of its own, counters reset before and compared after.  Returns {case: (errors, status)}."""
    cs, ex = table
    got = {}
    for c in cs:
        want = ex[c.name]
        eng.anim_counters(reset=True)
        errors, w_used, status = eng.anim_forced_rects(*ids[c.name], c.strand, c.rects)
        passes, calls = _counters(eng)
        where = (c.name, win_max, group_max)
        assert status.tolist() == [e["status"] for e in want], where
        assert errors.tolist() == [e["errors"] for e in want], where                                    # the host statement's ...
        assert all(g == e["ref_errors"] for g, e in zip(errors.tolist(), want) if e["status"] == 0), where      # ... and the referee's
        assert w_used.tolist() == [e["w_used"] for e in want], where
        want_passes, want_calls = fc.counters_of([e["spans"] for e in want], win_max, group_max)
        assert (passes, calls) == (want_passes, want_calls), (where, [e["spans"] for e in want])
        got[c.name] = (errors.tolist(), status.tolist())
    return got


@pytest.fixture(scope="module")
def default_run(table):
    """The table in the default configuration (checked against referee, host statement and counters): what the knob runs must repeat."""
    import os
    from pyani_amd.engine import Engine
    assert not any(k in os.environ for k in KNOBS)
    with Engine(0) as eng:
        return _run_table(eng, _load(eng, table[0]), table)


def test_every_case_against_referee_host_statement_and_counters(table, default_run):
    cs, ex = table
    assert set(default_run) == {c.name for c in cs}
    # the table as a whole: every kernel class counted, the group and the strips among them
    total_passes, total_calls = fc.counters_of([e["spans"] for c in cs for e in ex[c.name]])
    assert all(v > 0 for v in total_passes) and all(v > 0 for v in total_calls) and sum(total_passes) > sum(total_calls)


@pytest.mark.parametrize("win_max,group_max", [(256, 8184), (128, 8184), (2048, 0), (2048, 3064)])
def test_knob_configurations_move_the_runs_not_the_results(table, default_run, monkeypatch, win_max, group_max):
    """PYANI_PN_WINDOW_MAX caps the single-wave windows (wider runs go to the group of four waves), PYANI_PN_GROUP_MAX the group (wider
    runs go to the column strips): read when a context is created.  Same errors and status; the counters show where the passes ran."""
    from pyani_amd.engine import Engine
    if win_max != 2048:
        monkeypatch.setenv("PYANI_PN_WINDOW_MAX", str(win_max))
    if group_max != 8184:
        monkeypatch.setenv("PYANI_PN_GROUP_MAX", str(group_max))
    cs, ex = table
    runs = [e["spans"] for c in cs for e in ex[c.name]]
    base, moved = fc.counters_of(runs), fc.counters_of(runs, win_max, group_max)
    strips = lambda pc: sum(pc[0]) - sum(pc[1])      # noqa: E731  (passes without a diagonal-engine call)
    if group_max == 0:
        assert moved[1][3] == 0 and strips(moved) == strips(base) + base[1][3] > 0      # no pass on the group: all of them on the strips
    elif group_max == 3064:
        assert 0 < moved[1][3] < base[1][3] and strips(moved) > strips(base)
    else:
        assert moved[1][3] > base[1][3] and moved[1][1] + moved[1][2] < base[1][1] + base[1][2]      # off the wide windows, on to the group
    with Engine(0) as eng:
        got = _run_table(eng, _load(eng, cs), table, win_max, group_max)      # (asserts the moved counters case by case)
    assert got == default_run


def test_list_call_equals_single_calls_and_repeats(table):
    """A few hundred rectangles of every class in one call, in shuffled order, over both request lists (sum of sides above / up to
    1500): the rectangles' own answers, whatever stands next to them in the stream or in the list."""
    from pyani_amd.engine import Engine
    cs, ex = table
    with Engine(0) as eng:
        calls = []
        for strand in (0, 1):
            a, b, rects, who = fc.list_call(strand)
            calls.append((_add(eng, a), _add(eng, b), strand, rects, who))
        eng.upload()
        n, most, seen_status = 0, 0, set()
        for ra, qb, strand, rects, who in calls:
            eng.anim_counters(reset=True)
            first = eng.anim_forced_rects(ra, qb, strand, rects)
            passes, calls_ = _counters(eng)
            want = [ex[name][k] for name, k in who]
            assert first[2].tolist() == [e["status"] for e in want]
            assert first[0].tolist() == [e["errors"] for e in want]
            assert first[1].tolist() == [e["w_used"] for e in want]
            assert (passes, calls_) == fc.counters_of([e["spans"] for e in want])
            seen_status |= set(first[2].tolist())
            most = max(most, int(first[0].max()))
            again = eng.anim_forced_rects(ra, qb, strand, rects)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
            single = [eng.anim_forced_rects(ra, qb, strand, [r]) for r in rects]
            for j in range(3):
                assert [int(s[j][0]) for s in single] == first[j].tolist(), j
            n += len(rects)
        assert n >= 300 and seen_status == {0, 2} and most > 1000


def test_refusals_leave_the_engine_in_order(table, monkeypatch):
    from pyani_amd._lib import PG_E_ARG, PyaniGpuError
    from pyani_amd.engine import Engine
    cs, ex = table
    c = next(c for c in cs if c.name == "floor_C_ordinary")
    long_a, long_b, _, _ = fc.list_call(0)
    with Engine(0) as eng:
        ra, qb = _add(eng, c.a), _add(eng, c.b)
        la, lb = _add(eng, long_a), _add(eng, long_b)
        eng.upload()
        na, nb = len(c.a), len(c.b)
        bad = [(ra, qb, 0, [(10, 9, 0, 5)]),                      # N = 0
               (ra, qb, 0, [(0, 5, 7, 6)]),                       # M = 0
               (ra, qb, 0, [(0, 5, 0, 5), (50, 40, 0, 5)]),       # one bad rectangle refuses the call
               (ra, qb, 0, [(-1, 5, 0, 5)]), (ra, qb, 0, [(0, na, 0, 5)]), (ra, qb, 1, [(0, 5, -3, 5)]), (ra, qb, 1, [(0, 5, nb - 2, nb)]),
               (la, lb, 0, [(0, 10000, 0, 50)]), (la, lb, 0, [(0, 50, 100, 10100)]),      # a side of 10 001
               (ra, 9999, 0, [(0, 5, 0, 5)]), (-1, qb, 0, [(0, 5, 0, 5)]), (ra, qb, 2, [(0, 5, 0, 5)])]
        for args in bad:
            with pytest.raises(PyaniGpuError) as err:
                eng.anim_forced_rects(*args)
            assert err.value.code == PG_E_ARG, args
        lim = next(x for x in cs if x.name == "limit_longest_side")      # the longest side is taken: 10 000 x 50, the host statement's answer
        want = ex[lim.name][0]
        got = eng.anim_forced_rects(_add(eng, lim.a), _add(eng, lim.b), 0, lim.rects)
        assert (want["N"], want["M"]) == (10000, 50) and [int(x[0]) for x in got] == [want["errors"], want["w_used"], want["status"]]
        assert all(len(x) == 0 for x in eng.anim_forced_rects(ra, qb, 0, []))
        monkeypatch.delenv("PYANI_DEV_KNOBS")      # a development entry: refused without the switch
        with pytest.raises(PyaniGpuError) as err:
            eng.anim_forced_rects(ra, qb, 0, c.rects)
        assert err.value.code == PG_E_ARG
        monkeypatch.setenv("PYANI_DEV_KNOBS", "1")
        errors, w_used, status = eng.anim_forced_rects(ra, qb, 0, c.rects)
        assert (errors.tolist(), w_used.tolist(), status.tolist()) == ([30], [28], [0])
        assert ex[c.name][0]["errors"] == 30
        res = eng.anim_pairs([ra], [qb])      # an ordinary call afterwards: 1500 bases with 30 substitutions
        assert int(res["status"][0]) == 0 and 1400 <= int(res["ref_aln_len"][0]) <= 1500 and 25 <= int(res["sim_errors"][0]) <= 30
