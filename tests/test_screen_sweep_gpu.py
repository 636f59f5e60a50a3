"""GPU (through the C ABI): the sweep of the components over a ladder of thresholds (pg_screen_sweep / pg_screen_index_sweep / _read /
_read_snapshot / _last / _release; pyani_amd/csrc/pgscr_sweep.inc) against the numpy statement
(pyani_amd.screen.sweep_of_pairs, itself held to the tests' union-finds and to scipy by tests/test_screen_sweep_cpu.py).  Everything is an
integer and must be EQUAL: whatever the order of the list, the contention on a cell, the buckets' sizes, the upload chunks or the band
setting."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_components_cases as cc
from tests import screen_select_cases as ssc
from tests import screen_sweep_cases as swc

pytestmark = pytest.mark.gpu

BAND_ROWS = (1, 3, 8, 0)
NAMES = ("entries", "components", "singletons", "largest", "pair_slots")
NOTHING = {"n": 0, "steps": 0, "entries": 0, "ignored": 0, "level0": 0, "buckets": 0, "select_ms": 0.0, "sort_ms": 0.0, "hook_ms": 0.0, "census_ms": 0.0}


def _same_nodes(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.int32, np.uint64, np.uint64), ("root", "entries", "weight")):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def _same_sweep(got, want, what):
    for g, w, dtype, name in zip(got[:5], want[:5], (np.uint64, np.uint32, np.uint32, np.uint32, np.uint64), NAMES):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
    assert len(got[5]) == len(want[5]), (what, "snapshots")
    for k, (gn, wn) in enumerate(zip(got[5], want[5])):
        _same_nodes(gn, wn, (what, "snapshot", k))


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def small_engines():
    """{case: (engine, ids)} for family and edges: the genomes loaded once."""
    from pyani_amd.engine import Engine
    out, open_ = {}, []
    for case in ("family", "edges"):
        e = Engine(0).__enter__()
        open_.append(e)
        out[case] = (e, [e.add_genome(s, o) for s, o in scr.CASES[case]()])
    yield out
    for e in open_:
        e.__exit__(None, None, None)


_STATEMENTS = {}


def _statement(name):
    """sweep_of_pairs of a case: computed once, shared."""
    from pyani_amd import screen
    if name not in _STATEMENTS:
        a, b, s, level, n, steps, snaps = swc.CASES[name]()
        _STATEMENTS[name] = screen.sweep_of_pairs(a, b, level, n, steps, s, snaps)
    return _STATEMENTS[name]


# ---- the list entry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(swc.CASES))
def test_list_equals_the_statement(eng, name):
    a, b, s, level, n, steps, snaps = swc.CASES[name]()
    want = _statement(name)
    got = eng.screen_sweep(a, b, s, level, n=n, steps=steps, snapshots=snaps)
    _same_sweep(got, want, name)
    last = eng.screen_sweep_last()
    live = a != b
    assert (last["n"], last["steps"], last["entries"], last["ignored"]) == (n, steps, int(live.sum()), int((~live).sum())), last
    assert last["level0"] == int((level[live] == 0).sum()) and last["buckets"] == len(set(level[live].tolist()) - {0}), last
    assert last["select_ms"] == 0.0 and min(last["sort_ms"], last["hook_ms"], last["census_ms"]) >= 0.0
    if name == "chain_4095":
        assert got[1].tolist() == list(range(1, cc.CHAIN_N)) and last["buckets"] == swc.CHAIN_STEPS
    if name == "cliques_bridge":
        assert (got[4] == got[0]).tolist() == [step >= swc.BRIDGE_LEVEL for step in range(steps)]
    eng.screen_sweep_release()
    eng.screen_sweep_release()      # nothing resident: still fine
    assert eng.screen_sweep_last() == NOTHING


def test_snapshots_are_the_components_of_the_entries_present(eng):
    """The node arrays of a snapshot against components_of_pairs on the entries present there, and against the device's own components
    call; a step named twice is kept twice."""
    from pyani_amd import screen
    for name in ("chain_64", "buckets", "star"):
        a, b, s, level, n, steps, _ = swc.CASES[name]()
        snaps = (0, steps // 2, steps - 1, steps // 2)
        got = eng.screen_sweep(a, b, s, level, n=n, steps=steps, snapshots=snaps)
        for k, step in enumerate(snaps):
            here = level > step
            want = screen.components_of_pairs(a[here], b[here], s[here], n)
            _same_nodes(got[5][k], want, (name, step))
            _same_nodes(got[5][k], eng.screen_components(a[here], b[here], s[here], n=n), (name, step, "the device's components call"))
            assert got[1][step] == int((want[0] == np.arange(n)).sum())
    eng.screen_components_release()
    eng.screen_sweep_release()


def test_several_upload_chunks(eng, monkeypatch):
    """A list uploaded in pieces (the development knob cuts the chunk from 2^24 entries to 1000): the pieces are packed into one resident
    list, and the buckets are cut from the whole."""
    monkeypatch.setenv("PYANI_SWEEP_CHUNK", "1000")
    for name in ("cliques_bridge", "star"):
        a, b, s, level, n, steps, snaps = swc.CASES[name]()
        _same_sweep(eng.screen_sweep(a, b, s, level, n=n, steps=steps, snapshots=snaps), _statement(name), (name, "chunks of 1000"))
    eng.screen_sweep_release()


def test_refusals_leave_the_earlier_result(eng):
    from pyani_amd import _lib
    a, b, s, level, n, steps, snaps = swc.CASES["one_direction_duplicates"]()
    want = _statement("one_direction_duplicates")

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    def still_there(what):
        _same_sweep(eng._screen_sweep_read(n, steps, len(snaps)), want, what)
        assert {k: v for k, v in eng.screen_sweep_last().items() if not k.endswith("_ms")} == before, what

    eng.screen_sweep_release()
    refused(lambda: eng._screen_sweep_read(n, steps, 0), "no resident sweep")
    _same_sweep(eng.screen_sweep(a, b, s, level, n=n, steps=steps, snapshots=snaps), want, "before the refusals")
    before = {k: v for k, v in eng.screen_sweep_last().items() if not k.endswith("_ms")}
    one = ([1], [0], None, [1])
    for what, word, call in (
            ("no node", "nodes", lambda: eng.screen_sweep([], [], None, [], n=0, steps=2)),
            ("too many nodes", "nodes", lambda: eng.screen_sweep([], [], None, [], n=cc.MAX_N + 1, steps=2)),
            ("no step", "steps", lambda: eng.screen_sweep(*one, n=4, steps=0)),
            ("too many steps", "steps", lambda: eng.screen_sweep(*one, n=4, steps=4097)),
            ("33 snapshots", "snapshots", lambda: eng.screen_sweep(*one, n=4, steps=2, snapshots=[0] * 33)),
            ("a snapshot at steps", "snapshot", lambda: eng.screen_sweep(*one, n=4, steps=2, snapshots=[0, 2])),
            ("an index below", "outside", lambda: eng.screen_sweep([-1], [3], None, [1], n=8, steps=2)),
            ("an index at n", "outside", lambda: eng.screen_sweep([3], [8], None, [1], n=8, steps=2)),
            ("a level above the steps", "level", lambda: eng.screen_sweep([1, 2], [0, 0], None, [2, 3], n=4, steps=2)),
            ("a NULL array", "NULL", lambda: eng._check(eng.lib.pg_screen_sweep(eng._h, None, None, None, None, 1, 4, 2, None, 0))),
            ("a NULL level", "NULL", lambda: eng._check(eng.lib.pg_screen_sweep(eng._h, np.zeros(1, np.int32).ctypes.data, np.ones(1, np.int32).ctypes.data, None, None, 1, 4, 2, None, 0))),
            ("no resident index", "no resident index", lambda: eng.screen_index_sweep(np.zeros((2, 3), np.uint32))),
            ("no such snapshot", "does not exist", lambda: eng._check(eng.lib.pg_screen_sweep_read_snapshot(eng._h, len(snaps), *(np.zeros(n, dt).ctypes.data for dt in (np.int32, np.uint64, np.uint64)))))):
        refused(call, word)
        still_there(("after", what))
    # independent of the resident matrix and of the components: a load, a selection, their release and a components call leave the sweep alone
    sizes, loaded = ssc.random_symmetric(13, 70)
    eng.screen_load(loaded)
    eng.screen_select(np.full(70, 3, dtype=np.uint32))
    eng.screen_release()
    eng.screen_components(a, b, s, n=n)
    eng.screen_components_release()
    still_there("after the resident matrix and the components came and went")
    eng.screen_sweep_release()
    eng.screen_sweep_release()
    refused(lambda: eng._screen_sweep_read(n, steps, 0), "no resident sweep")
    assert eng.screen_sweep_last() == NOTHING


# ---- the index entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_index_sweep_equals_the_list_and_the_per_step_route(small_engines, case, k, scale):
    """The index form against the list form over the list screen_candidates returns at T_0 with sweep_levels' levels, and every step's
    snapshot against what screen_components_of returns at that threshold — the route of one call per step, which shares no new code."""
    from pyani_amd import screen
    e, ids = small_engines[case]
    n, steps = len(ids), len(swc.LADDER)
    snaps = tuple(range(steps))
    per_step = [e.screen_components_of(ids, screen.ScreenOptions(t, k, scale, 2), path="index") for t in swc.LADDER]
    assert len({len(c.size) for c in per_step}) >= 2      # the ladder moves the components
    kept = e.screen_candidates(ids, screen.ScreenOptions(swc.LADDER[0], k, scale, 2))
    need = screen.sweep_thresholds(kept.sizes, k, swc.LADDER, 2)
    level = screen.sweep_levels(kept.a, kept.b, kept.shared, need)
    of_list = e.screen_sweep(kept.a, kept.b, kept.shared, level, n=n, steps=steps, snapshots=snaps)
    _same_sweep(of_list, screen.sweep_of_pairs(kept.a, kept.b, level, n, steps, kept.shared, snaps), (case, "the list form"))
    try:
        for setting in BAND_ROWS:
            e.screen_set_band(setting)
            sizes = e.screen_index(ids, kmer=k, scale=scale)
            assert (sizes == kept.sizes).all()
            a, b, s = e.screen_index_select(need[0])
            before = e.screen_index_last()
            *got, n_pairs = e.screen_index_sweep(need, snapshots=snaps)
            assert n_pairs == len(a) == len(kept.a), (case, setting, n_pairs, len(a))
            _same_sweep(got, of_list, (case, setting))
            last = e.screen_sweep_last()
            assert (last["n"], last["steps"], last["entries"], last["ignored"], last["level0"]) == (n, steps, len(a), 0, 0), last
            assert last["buckets"] == len(set(level.tolist())) and last["select_ms"] > 0.0
            for step in snaps:
                for g, w in zip(got[5][step], (per_step[step].root, per_step[step].entries, per_step[step].weight)):
                    assert g.dtype == w.dtype and (g == w).all(), (case, setting, step)
                assert got[1][step] == len(per_step[step].size) and got[3][step] == per_step[step].size.max()
                assert bool(got[4][step] == got[0][step]) == bool(per_step[step].complete.all()), (case, setting, step)
            # the index, its selection and its counters are as pg_screen_index_select left them
            now = e.screen_index_last()
            assert {x: now[x] for x in now if not x.endswith("_ms")} == {x: before[x] for x in before if not x.endswith("_ms")}
            sel = [np.zeros(len(a), dt) for dt in (np.int32, np.int32, np.uint32)]
            e._check(e.lib.pg_screen_index_read(e._h, *(x.ctypes.data if len(a) else None for x in sel)))
            assert all((x == y).all() for x, y in zip(sel, (a, b, s)))
    finally:
        e.screen_set_band(0)
        e.screen_index_release()
        e.screen_sweep_release()


def test_index_refusals(small_engines):
    from pyani_amd import _lib, screen
    e, ids = small_engines["edges"]
    k, scale = scr.EDGES_PARAMS
    n = len(ids)

    def refused(call, word):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG and word in str(err.value), str(err.value)

    try:
        sizes = e.screen_index(ids, kmer=k, scale=scale)
        need = screen.sweep_thresholds(sizes, k, swc.LADDER, 2)
        *want, _ = e.screen_index_sweep(need, snapshots=(0,))
        before = {x: v for x, v in e.screen_sweep_last().items() if not x.endswith("_ms")}
        falling = need.copy()
        falling[3, 2] = falling[2, 2] - 1 if falling[2, 2] else 0
        falling[2, 2] += 1
        for what, word, call in (
                ("a table that falls", "not monotone", lambda: e.screen_index_sweep(falling)),
                ("another n", "genomes", lambda: e.screen_index_sweep(need[:, :-1])),
                ("33 snapshots", "snapshots", lambda: e.screen_index_sweep(need, snapshots=[0] * 33)),
                ("a snapshot at steps", "snapshot", lambda: e.screen_index_sweep(need, snapshots=[len(need)])),
                ("a table beyond a gigabyte", "2^28", lambda: e._check(e.lib.pg_screen_index_sweep(e._h, need.ctypes.data, (1 << 16) + 1, 4096, 0, 1, None, 0, None))),
                ("no step", "steps", lambda: e._check(e.lib.pg_screen_index_sweep(e._h, need.ctypes.data, n, 0, 0, 1, None, 0, None))),
                ("too many steps", "steps", lambda: e._check(e.lib.pg_screen_index_sweep(e._h, need.ctypes.data, n, 4097, 0, 1, None, 0, None)))):
            refused(call, word)
            _same_sweep(e._screen_sweep_read(n, len(need), 1), want, ("after", what))
            assert {x: v for x, v in e.screen_sweep_last().items() if not x.endswith("_ms")} == before
    finally:
        e.screen_index_release()
        e.screen_sweep_release()


def test_sweep_of_dense_and_index_are_equal(small_engines):
    from pyani_amd import screen
    e, ids = small_engines["family"]
    labels = [f"g{i}" for i in range(len(ids))]
    opt = screen.ScreenOptions(0.5, 16, 16)      # (its min_identity is ignored in favour of the ladder)
    dense = e.screen_sweep_of(ids, opt, swc.LADDER, labels=labels, path="dense", snapshots=(0, 4))
    index = e.screen_sweep_of(ids, opt, swc.LADDER, labels=labels, path="index", snapshots=(0, 4))
    host = e.screen_candidates(ids, screen.ScreenOptions(swc.LADDER[0], 16, 16), labels=labels).sweep(swc.LADDER, (0, 4))      # engine=None: the statement
    for other in (index, host):
        assert other.labels == dense.labels == labels and other.snapshot_steps == dense.snapshot_steps == [0, 4]
        for f in ("identities", "entries", "components", "singletons", "largest", "pair_slots", "complete"):
            x, y = getattr(other, f), getattr(dense, f)
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), f
        for step in (0, 4):
            for f in screen.ScreenComponents._fields[1:]:
                assert (getattr(other.components_at(step), f) == getattr(dense.components_at(step), f)).all(), (step, f)
    assert len(set(dense.components.tolist())) >= 2
    assert e.screen_sweep_last() == NOTHING      # nothing stays resident
    with pytest.raises(Exception):
        e.screen_index_band(0)


def test_run_screen_sweep(tmp_path):
    import pandas as pd
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_screen import run_screen, tab_path
    indir = tmp_path / "in"
    indir.mkdir()
    for i, (seq, off) in enumerate(scr.family()):
        synth.write_fasta(indir / f"g{i}.fna", seq, off, f"g{i}")
    with Engine(0) as e:
        plain = run_screen(indir, tmp_path / "plain", scale=16, min_identity=0.8, write_output=True, engine=e)
        assert plain.sweep is None and not tab_path(tmp_path / "plain", "sweep").exists()
        run = run_screen(indir, tmp_path / "out", scale=16, write_output=True, engine=e, sweep=swc.LADDER)
        assert e.genome_count() == 0 and e.screen_sweep_last() == NOTHING
    assert run.screened is None and run.sweep.labels == [f"g{i}" for i in range(8)]
    assert sorted(p.name for p in (tmp_path / "out" / "screen_output").iterdir()) == [f"screen_{x}.tab" for x in ("containment", "identity", "shared", "sweep")]
    frame = run.sweep.frame()
    again = pd.read_csv(tab_path(tmp_path / "out", "sweep"), sep="\t", float_precision="round_trip")
    assert list(again.columns) == list(frame.columns) and len(again) == len(swc.LADDER)
    for col in frame.columns:
        assert again[col].tolist() == frame[col].tolist(), col
    assert frame["entries"].tolist()[0] == len(plain.screened.a) and len(set(frame["components"].tolist())) >= 2
