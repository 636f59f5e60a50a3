"""GPU: every trimmed-search engine of the ANIm extender on the directed searches of tests/search_cases.py, through the development
entry pg_anim_searches — the pre-pass kernels' engine (256-diagonal window, overflow reported), the walks' engine (the ladder 256 ->
512 -> global memory), each rung of that ladder called directly, and the one-gap-per-lane kernels through the batch's own gap
launches.  Every comparison is exact, against pgn::ScalarEngine and the independent restatement's align_engine (tests/search_cases.py
expected(); tests/test_searches_cpu.py holds the two against each other and the table against its claims), and the engine counters
(pg_anim_counters: calls, window moves, window misfits, global-engine calls) against what the host emulation of the window did."""
import numpy as np
import pytest

from tests import search_cases as sc

pytestmark = pytest.mark.gpu

GLOBAL_MAX_SIDE = 3000      # the global-memory engine is slow by design: called directly only on searches up to this size


@pytest.fixture(scope="module")
def table():
    return sc.cases(), sc.expected()


def _add(eng, seq):
    return eng.add_genome(np.frombuffer(seq.encode(), dtype=np.uint8), np.array([0, len(seq)], dtype=np.uint64))


@pytest.fixture(scope="module")
def loaded(table):
    """One engine with every case's two sequences resident, and the results of the single calls made so far: {engine: {case: rows}}."""
    from pyani_amd.engine import Engine
    with Engine(0) as eng:
        ids = {c.name: (_add(eng, c.a), _add(eng, c.b)) for c in table[0]}
        eng.upload()
        yield eng, ids, {}


def _counters(eng):
    c = [int(v) for v in eng.anim_counters()]
    return dict(diag_calls=c[0], moves=c[9], misfits=c[10], global_calls=c[6])


def _single_calls(loaded, table, engine, only=lambda c, e: True):
    """Every case in a call of its own on `engine` (the searches `only` lets through), counters reset before and read after.  Checks rows and
    counters against the expectations and returns {case: {search index: row}}."""
    eng, ids, done = loaded
    if engine in done:
        return done[engine]
    cs, ex = table
    got = {}
    for c in cs:
        ks = [k for k, e in enumerate(ex[c.name]) if only(c, e)]
        if not ks:
            continue
        eng.anim_counters(reset=True)
        rows = eng.anim_searches(*ids[c.name], c.strand, engine, [c.searches[k] for k in ks])
        cnt = _counters(eng)
        es = [ex[c.name][k] for k in ks]
        where = (engine, c.name)
        assert [tuple(r) for r in rows.tolist()] == [sc.want(e, engine) for e in es], where            # the scalar engine's ...
        assert all(tuple(r[:4]) == e["oracle"] for r, e in zip(rows.tolist(), es) if r[4]), where      # ... and the independent restatement's
        # what the engines did: the window moves of the emulation (on the window that held the search), the windows that did not hold
        # it, the calls that went on to global memory
        f4, f8 = [e["e4"]["fit"] for e in es], [e["e8"]["fit"] for e in es]
        if engine in ("PREPASS", "RUNG_256"):
            want = dict(diag_calls=sum(f4), moves=sum(e["e4"]["moves"] for e in es if e["e4"]["fit"]), misfits=len(es) - sum(f4), global_calls=0)
        elif engine == "RUNG_512":
            want = dict(diag_calls=sum(f8), moves=sum(e["e8"]["moves"] for e in es if e["e8"]["fit"]), misfits=len(es) - sum(f8), global_calls=0)
        elif engine == "WALK":      # 256 first; what it does not hold starts over on 512; what that does not hold either goes to global memory
            want = dict(diag_calls=sum(f8), moves=sum(e["e4"]["moves"] if e["e4"]["fit"] else e["e8"]["moves"] for e in es if e["e8"]["fit"]),
                        misfits=2 * len(es) - sum(f4) - sum(f8), global_calls=len(es) - sum(f8))
        else:
            want = dict(diag_calls=0, moves=0, misfits=0, global_calls=len(es))
        assert cnt == want, where
        got[c.name] = {k: tuple(r) for k, r in zip(ks, rows.tolist())}
    done[engine] = got
    return got


@pytest.mark.parametrize("engine", ["WALK", "PREPASS"])
def test_walk_and_prepass_on_every_case(loaded, table, engine):
    """WALK holds everything (the band that outgrows 256 diagonals starts over on 512, what outgrows those on global memory: the counters
    show both hand-overs taken); PREPASS reports exactly the searches whose band the emulated 256-diagonal window did not hold, with
    zeros, and the other searches of the same call are the scalar engine's."""
    cs, ex = table
    got = _single_calls(loaded, table, engine)
    assert set(got) == {c.name for c in cs}
    held = [r[4] for c in cs for r in got[c.name].values()]
    n_misfit = sum(1 - e["e4"]["fit"] for c in cs for e in ex[c.name])
    assert n_misfit >= 40
    assert sum(held) == len(held) - (n_misfit if engine == "PREPASS" else 0)


@pytest.mark.parametrize("engine", ["RUNG_256", "RUNG_512"])
def test_each_window_alone_on_every_case(loaded, table, engine):
    """pn_align_diag<4> / <8> called directly: held is the emulation's fit, the result the scalar engine's, the window moved as often
    as the emulation's (tests/test_searches_cpu.py: the drift cases move it, in both directions)."""
    cs, ex = table
    got = _single_calls(loaded, table, engine)
    key = "e4" if engine == "RUNG_256" else "e8"
    assert sum(r[4] for c in cs for r in got[c.name].values()) == sum(e[key]["fit"] for c in cs for e in ex[c.name])
    assert sum(e[key]["moves"] for c in cs for e in ex[c.name]) > 0


def test_global_memory_engine_alone(loaded, table):
    """pn_align_wave<true> called directly on every search with sides up to 3000 bases — the outgrow cases among them, whose widest
    anti-diagonals (up to ~290 cells) take five trips of the wave."""
    cs, ex = table
    got = _single_calls(loaded, table, "RUNG_GLOBAL", lambda c, e: max(e["N"], e["M"]) <= GLOBAL_MAX_SIDE)
    assert {c.name for c in cs if c.group == "outgrow"} <= set(got)
    assert sum(len(g) for g in got.values()) >= 3000 and max(ex[n][k]["wmax"] for n, g in got.items() for k in g) > 256


def test_the_walk_takes_the_first_rung_that_holds(loaded, table):
    cs, ex = table
    walk = _single_calls(loaded, table, "WALK")
    rungs = [_single_calls(loaded, table, "RUNG_256"), _single_calls(loaded, table, "RUNG_512"),
             _single_calls(loaded, table, "RUNG_GLOBAL", lambda c, e: max(e["N"], e["M"]) <= GLOBAL_MAX_SIDE)]
    first = [0, 0, 0]
    for c in cs:
        for k, row in walk[c.name].items():
            t = next(t for t, r in enumerate(rungs) if k in r.get(c.name, {}) and r[c.name][k][4])
            assert row == rungs[t][c.name][k], (c.name, k, t)
            first[t] += 1
    assert all(first), first      # every rung was the first to hold for some search


def test_lane_kernels_and_the_gap_launches(loaded, table):
    """Every lanes case through launch_gaps: small gaps are answered by the lane kernel of their size class (the scalar engine's result =
    the plain untrimmed global alignment's error count), the 60-base ones by the wave kernel; lists of 64 k + 1 gaps to the last one."""
    eng, ids, _ = loaded
    cs, ex = table
    n_small = n_big = 0
    for c in cs:
        if not c.lanes:
            continue
        eng.anim_counters(reset=True)
        rows = [tuple(r) for r in eng.anim_searches(*ids[c.name], c.strand, "LANES", c.searches).tolist()]
        # the wave kernel (counter class 0: the diagonal engine's calls in the gaps kernel) ran the gaps that are not small and no others
        assert int(eng.anim_counters()[32]) == sum(sc.lane_class(e["N"], e["M"]) is None for e in ex[c.name]), c.name
        for k, (row, e) in enumerate(zip(rows, ex[c.name])):
            assert row == e["scalar"] + (1,) == e["oracle"] + (1,), (c.name, k, e["N"], e["M"])
            if sc.lane_class(e["N"], e["M"]):
                assert row[2] == e["global_errors"] and row[3] == 1 and row[:2] == c.searches[k][2:4], (c.name, k)
                n_small += 1
            else:
                n_big += 1
        if c.name.startswith("lanes_list_"):
            assert len(rows) % 64 == 1 and rows[-1][4] == 1
    assert n_small >= 1000 and n_big >= 20


@pytest.mark.parametrize("engine", ["WALK", "PREPASS", "LANES"])
def test_list_call_equals_single_calls_and_repeats(table, engine):
    """All cases of a strand back to back in one stream pair, all their searches in one call in shuffled order (this is what runs the
    cursors' chunking: 8 / 4 / 8 items a turn in PREPASS, lists of a thousand gaps over the lane classes in LANES): every search's own
    answer — the one its single call gave (both are held to the same expectation) — whatever stands next to it, and the same bytes again."""
    from pyani_amd.engine import Engine
    cs, ex = table
    with Engine(0) as eng:
        calls = []
        for strand in (0, 1):
            a, b, searches, who = sc.list_call(strand, lanes=engine == "LANES")
            calls.append((_add(eng, a), _add(eng, b), strand, searches, who))
        eng.upload()
        n = n_unheld = 0
        for ra, qb, strand, searches, who in calls:
            first = eng.anim_searches(ra, qb, strand, engine, searches)
            got = [tuple(r) for r in first.tolist()]      # (ends come back as positions of the joined streams)
            got = [(g[0] - a_off, g[1] - b_off) + g[2:] if g[4] else g for g, (_, _, a_off, b_off) in zip(got, who)]
            want = [sc.want(ex[name][k], engine) for name, k, _, _ in who]
            bad = [(w, g, x) for w, g, x in zip(who, got, want) if g != x]
            assert not bad, bad[:5]
            assert first.tobytes() == eng.anim_searches(ra, qb, strand, engine, searches).tobytes()
            n += len(searches)
            n_unheld += sum(1 - g[4] for g in got)
            # a search that was not held stands next to searches that were: theirs are unaffected (asserted above), it is all zeros
            assert all(g == (0, 0, 0, 0, 0) for g in got if not g[4])
        assert n >= (1000 if engine == "LANES" else 3000)
        assert (n_unheld > 0) == (engine != "WALK")


def test_refusals_leave_the_engine_in_order(table, monkeypatch):
    from pyani_amd._lib import PG_E_ARG, PyaniGpuError
    from pyani_amd.engine import Engine
    cs, ex = table
    rng = np.random.default_rng(4603)
    a = sc.rand_seq(rng, 1500)
    b = sc.substitute(rng, a, range(24, 1500, 50))      # 30 substitutions
    long_a, long_b, _, _ = sc.list_call(0)
    F, B, O = sc.FORWARD_ALIGN, sc.BACKWARD_SEARCH, sc.OPTIMAL_BIT
    with Engine(0) as eng:
        ra, qb = _add(eng, a), _add(eng, b)
        la, lb = _add(eng, long_a), _add(eng, long_b)
        eng.upload()
        na, nb = len(a), len(b)
        ok = (0, 0, 99, 99, F)
        bad = [(ra, qb, 0, "WALK", [(0, 0, 99, 99, 5)]),                         # FORCED_BIT: a forced run is no search
               (ra, qb, 0, "WALK", [(0, 0, 99, 99, F | 4 | O)]),
               (ra, qb, 0, "WALK", [(0, 0, 99, 99, 0)]), (ra, qb, 0, "WALK", [(0, 0, 99, 99, 3)]), (ra, qb, 0, "WALK", [(0, 0, 99, 99, 17)]),      # no mode of the four
               (ra, qb, 0, "PREPASS", [(-1, 0, 99, 99, F)]), (ra, qb, 0, "PREPASS", [(0, 0, na, 99, F)]), (ra, qb, 1, "WALK", [(0, -2, 99, 99, F)]),
               (ra, qb, 1, "RUNG_256", [(0, 0, 99, nb, F)]), (ra, qb, 0, "RUNG_GLOBAL", [(99, 99, 0, -1, B)]), (ra, qb, 0, "WALK", [(na, 99, 0, 0, B)]),      # outside its stream
               (ra, qb, 0, "WALK", [(50, 0, 49, 99, F)]), (ra, qb, 0, "WALK", [(0, 50, 99, 49, F | O)]),      # the target before the start, forwards
               (ra, qb, 0, "WALK", [(49, 99, 50, 0, B)]), (ra, qb, 0, "RUNG_512", [(99, 49, 0, 50, B | O)]),      # ... behind it, backwards
               (ra, qb, 0, "WALK", [ok, (50, 0, 49, 99, F)]),                     # one bad search refuses the call
               (la, lb, 0, "WALK", [(0, 0, 10000, 50, F)]), (la, lb, 0, "PREPASS", [(50, 10100, 0, 100, B)]),      # a side of 10 001
               (ra, 9999, 0, "WALK", [ok]), (-1, qb, 0, "WALK", [ok]), (ra, qb, 2, "WALK", [ok]), (ra, qb, 0, 6, [ok]), (ra, qb, 0, -1, [ok]),
               (ra, qb, 0, "LANES", [(0, 0, 20, 20, F | O)]), (ra, qb, 0, "LANES", [(20, 20, 0, 0, B)])]      # LANES: match-to-match gaps only
        for args in bad:
            with pytest.raises(PyaniGpuError) as err:
                eng.anim_searches(*args)
            assert err.value.code == PG_E_ARG, args
        assert [tuple(r) for r in eng.anim_searches(la, lb, 0, "WALK", [(0, 0, 9999, 50, F)]).tolist()][0][4] == 1      # the longest side is taken
        assert eng.anim_searches(ra, qb, 0, "WALK", []).shape == (0, 5)
        ticket = eng.anim_pairs_enqueue([ra], [qb])      # refused while an enqueued call is in flight (until it is fetched)
        with pytest.raises(PyaniGpuError) as err:
            eng.anim_searches(ra, qb, 0, "WALK", [ok])
        assert err.value.code == PG_E_ARG
        eng.anim_pairs_fetch(ticket)
        monkeypatch.delenv("PYANI_DEV_KNOBS")      # a development entry: refused without the switch
        with pytest.raises(PyaniGpuError) as err:
            eng.anim_searches(ra, qb, 0, "WALK", [ok])
        assert err.value.code == PG_E_ARG
        monkeypatch.setenv("PYANI_DEV_KNOBS", "1")
        for engine in ("WALK", "PREPASS", "RUNG_256", "RUNG_512", "RUNG_GLOBAL"):
            rows = eng.anim_searches(ra, qb, 0, engine, [(0, 0, na - 1, nb - 1, F), (na - 1, nb - 1, 0, 0, B)])
            assert [tuple(r) for r in rows.tolist()] == [(na - 1, nb - 1, 30, 1, 1), (0, 0, 30, 1, 1)], engine
        assert [tuple(r) for r in eng.anim_searches(ra, qb, 0, "LANES", [(0, 0, 58, 58, F), (0, 0, 99, 99, F)]).tolist()] == [(58, 58, 1, 1, 1), (99, 99, 2, 1, 1)]
        res = eng.anim_pairs([ra], [qb])      # an ordinary call afterwards: 1500 bases with 30 substitutions
        assert int(res["status"][0]) == 0 and 1400 <= int(res["ref_aln_len"][0]) <= 1500 and 25 <= int(res["sim_errors"][0]) <= 30
