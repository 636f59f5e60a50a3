"""GPU: neighbour joining through the C ABI (pg_tree_nj / pg_tree_nj_set / pg_tree_nj_last) EQUALS the statement
(pyani_amd.tree.nj_of_matrix): integers equal, doubles bit for bit, on every case of tests/tree_cases.py; no case is skipped.

Sizes: 3, 4, 5; 63 / 64 / 65 and 127 / 129 / 130 round the 64-wide tiles of the arg-min; 257 and 700 as the large ones (700: 66 tiles, the
statement takes about a second, computed once).  Every case runs under tail_limit 3 (every step wide: arg-min, join and compaction
at small n), 4, 64 and the default 512; the hand-over is also taken at tail_limit = n - 1, n and n + 1.  The join and tail workgroup
has 1024 threads: its loops' second rounds begin at 1025 live nodes or partials, beyond what the statement reaches in seconds, so the
large cases also run with the workgroup narrowed to 64 and 256 threads (the development knob PYANI_TREE_WG), where 700 nodes and 66
partials take up to eleven rounds of the same loops.  The counters must report the cells scanned as the sum over the wide steps of
m (m - 1) / 2: dead slots are not scanned.  Refusals leave the outputs untouched."""

import numpy as np
import pandas as pd
import pytest

from tests import tree_cases as tc

pytestmark = pytest.mark.gpu

DEFAULT_TAIL = 512
TAILS = (3, 4, 64, DEFAULT_TAIL)
ALL_CASES = tc.SMALL + sorted(tc.LARGE)


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


def expected_counts(n, tail):
    wide = max(n - max(tail, 3), 0)
    cells = sum(m * (m - 1) // 2 for m in range(n, n - wide, -1))
    return {"n": n, "wide_steps": wide, "tail_steps": n - 3 - wide, "launches": 2 + 2 * wide + 1, "cells_scanned": cells}


def run(eng, name, tail):
    eng.tree_nj_set(tail)
    got = eng.tree_nj(tc.matrix(name))
    counts, _ = eng.tree_nj_last()
    eng.tree_nj_set(DEFAULT_TAIL)
    return got, counts


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_device_equals_statement(eng, name, tail):
    got, counts = run(eng, name, tail)
    want = tc.statement(name)
    assert np.array_equal(got[0], want.joins) and np.array_equal(got[2], want.last), f"{name} tail_limit {tail}: joins differ"
    assert tc.same_tree(got, tc.tree_arrays(want)), f"{name} tail_limit {tail}: lengths differ"
    assert got[0].dtype == np.int32 and got[2].dtype == np.int32
    assert counts == expected_counts(len(tc.matrix(name)), tail)


@pytest.mark.parametrize("name", sorted(tc.ADDITIVE))
def test_additive_matrices_give_their_tree_back(eng, name):
    from pyani_amd import tree
    g, D = tc.additive(name)
    got, _ = run(eng, name, 3)
    t = tree.Tree(len(D), *got)
    assert t.splits() == tc.graph_splits(g, t.n) and tc.same_bits(t.patristic(), D)


@pytest.mark.parametrize("name", ["n5", "dup21", "int33", "add33", "rand65", "equal65", "rand129"])
def test_hand_over_round_the_tail_limit(eng, name):
    n = len(tc.matrix(name))
    want = tc.tree_arrays(tc.statement(name))
    for tail in (n - 1, n, n + 1):
        if tail < 3:
            continue
        got, counts = run(eng, name, tail)
        assert tc.same_tree(got, want), f"{name}: tail_limit {tail}"
        assert counts == expected_counts(n, tail)


@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("name,tail", [("rand700", 3), ("rand700", 650), ("ident257", 3), ("ident257", 200), ("rand129", 3)])
def test_later_rounds_of_the_workgroup_loops(eng, monkeypatch, name, tail, threads):
    monkeypatch.setenv("PYANI_TREE_WG", str(threads))
    got, counts = run(eng, name, tail)
    assert tc.same_tree(got, tc.tree_arrays(tc.statement(name))), f"{name}: {threads} threads, tail_limit {tail}"
    assert counts == expected_counts(len(tc.matrix(name)), tail)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_call(eng, d, n, outs):
    return eng.lib.pg_tree_nj(eng._h, None if d is None else d.ctypes.data, n, *(None if o is None else o.ctypes.data for o in outs))


def sentinels(n):
    k = max(n - 3, 1)
    return [np.full((k, 2), -7, dtype=np.int32), np.full((k, 2), -7.5), np.full(3, -7, dtype=np.int32), np.full(3, -7.5)]


def untouched(outs):
    return all((o == (-7 if o.dtype == np.int32 else -7.5)).all() for o in outs)


def check_works(eng, name="int33"):
    got, _ = run(eng, name, DEFAULT_TAIL)
    assert tc.same_tree(got, tc.tree_arrays(tc.statement(name)))


@pytest.mark.parametrize("name", ["asymmetric", "signed_zero", "diagonal", "nan", "inf", "overflow", "overflow_q", "overflow_later"])
@pytest.mark.parametrize("tail", [3, DEFAULT_TAIL])
def test_bad_matrices_are_refused_and_leave_the_outputs(eng, name, tail):
    from pyani_amd import _lib
    d = np.ascontiguousarray(tc.bad_inputs()[name])
    want = _lib.PG_E_ARG if name in ("asymmetric", "signed_zero", "diagonal") else _lib.PG_E_NONFINITE
    outs = sentinels(len(d))
    eng.tree_nj_set(tail)
    assert raw_call(eng, d, len(d), outs) == want and untouched(outs)
    assert eng.lib.pg_last_error(eng._h).decode().startswith("tree:")
    with pytest.raises(_lib.PyaniGpuError) as err:
        eng.tree_nj(d)
    assert err.value.code == want
    check_works(eng)      # a call after a refused one


def test_bad_sizes_and_null_are_refused(eng):
    from pyani_amd import _lib
    eng.tree_nj_set(DEFAULT_TAIL)
    ok = np.ascontiguousarray(tc.matrix("n5"))
    for d, n in ((ok, 2), (ok, 0), (None, 5), (np.zeros((8193, 8193)), 8193)):      # the zeros are never touched: the size is checked first
        outs = sentinels(5)
        assert raw_call(eng, d, n, outs) == _lib.PG_E_ARG and untouched(outs)
    with pytest.raises(_lib.PyaniGpuError) as err:
        eng.tree_nj(np.zeros((2, 2)))
    assert err.value.code == _lib.PG_E_ARG
    with pytest.raises(ValueError):
        eng.tree_nj(np.zeros((3, 4)))
    check_works(eng)


def test_tail_limit_outside_its_range_is_refused_and_changes_nothing(eng):
    from pyani_amd import _lib
    eng.tree_nj_set(7)
    for bad in (0, 2, 1025, 1 << 20):
        with pytest.raises(_lib.PyaniGpuError) as err:
            eng.tree_nj_set(bad)
        assert err.value.code == _lib.PG_E_ARG
    eng.tree_nj(tc.matrix("int33"))
    assert eng.tree_nj_last()[0] == expected_counts(33, 7)
    eng.tree_nj_set(3), eng.tree_nj_set(1024), eng.tree_nj_set(DEFAULT_TAIL)


# ---- call hygiene ---------------------------------------------------------------------------------------------------------------------
def test_null_outputs_are_accepted(eng):
    eng.tree_nj_set(DEFAULT_TAIL)
    d = np.ascontiguousarray(tc.matrix("rand65"))
    want = tc.tree_arrays(tc.statement("rand65"))
    assert raw_call(eng, d, 65, [None] * 4) == 0
    for keep in range(4):
        outs = sentinels(65)
        assert raw_call(eng, d, 65, [o if k == keep else None for k, o in enumerate(outs)]) == 0
        if outs[keep].dtype == np.int32:
            assert np.array_equal(outs[keep], want[keep])
        else:
            assert tc.same_bits(outs[keep], want[keep])
    assert eng.lib.pg_tree_nj_last(eng._h, None, None) == 0


def test_two_calls_give_the_same_bits_and_the_stage_times_follow_profiling(eng):
    first, _ = run(eng, "ident257", 64)
    second, _ = run(eng, "ident257", 64)
    assert tc.same_tree(first, second)
    assert eng.tree_nj_last()[1] == {"validate_ms": 0.0, "wide_ms": 0.0, "tail_ms": 0.0}      # profiling is off
    eng.profile_enable(True)
    try:
        third, _ = run(eng, "ident257", 64)
        ms = eng.tree_nj_last()[1]
    finally:
        eng.profile_enable(False)
    assert tc.same_tree(first, third) and all(v > 0.0 for v in ms.values())
    assert eng.tree_nj_last()[1] == {"validate_ms": 0.0, "wide_ms": 0.0, "tail_ms": 0.0}


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def test_neighbor_joining_on_a_frame_equals_the_engine_call(eng):
    from pyani_amd import tree
    D = tc.matrix("ident70")
    names = [f"genome_{i}" for i in range(70)]
    frame = pd.DataFrame(1.0 - D, index=names, columns=names)
    got = tree.neighbor_joining(frame, kind="identity", engine=eng)
    direct = eng.tree_nj(tree.distances_of(frame, kind="identity"))
    assert tc.same_tree(tc.tree_arrays(got), direct) and got.labels == names and got.n == 70
    assert tc.same_tree(direct, tc.tree_arrays(tree.nj_of_matrix(tree.distances_of(frame, kind="identity"))))
    asym = frame.copy()
    asym.iloc[3, 9] -= 0.01      # an ANIb-like matrix: the two directions differ
    for sym in ("mean", "min", "max"):
        t = tree.neighbor_joining(asym, kind="identity", symmetrize=sym, engine=eng)
        assert tc.same_tree(tc.tree_arrays(t), tc.tree_arrays(tree.nj_of_matrix(tree.distances_of(asym, kind="identity", symmetrize=sym))))
    with pytest.raises(ValueError):
        tree.neighbor_joining(tc.bad_inputs()["overflow"], engine=eng)
    with pytest.raises(ValueError):
        tree.neighbor_joining(tc.bad_inputs()["overflow_q"], engine=eng)      # finite cells: the device's own refusal


def test_multi_engine_equals_engine(eng):
    from pyani_amd.multi import MultiEngine
    D = tc.matrix("rand129")
    with MultiEngine([0, 0]) as multi:
        multi.tree_nj_set(64)
        got = multi.tree_nj(D)
        assert multi.tree_nj_last()[0] == expected_counts(129, 64)
    assert tc.same_tree(got, eng.tree_nj(D)) and tc.same_tree(got, tc.tree_arrays(tc.statement("rand129")))


def test_run_tree_writes_files_that_read_back_to_the_same_tree(eng, tmp_path):
    from pyani_amd import tree
    D = tc.matrix("dup70")
    names = [f"strain {i}" for i in range(70)]
    tab = tmp_path / "matrix_identity.tab"
    pd.DataFrame(D, index=names, columns=names).to_csv(tab, index=True, sep="\t")
    run_ = tree.run_tree(tab, tmp_path, engine=eng)
    want = tc.statement("dup70")
    assert tc.same_tree(tc.tree_arrays(run_.tree), tc.tree_arrays(want))
    assert run_.newick_path == tmp_path / "tree_output" / "matrix_identity_nj.nwk" and run_.edges_path == tmp_path / "tree_output" / "matrix_identity_nj_edges.tab"
    assert tc.newick_matches(want, run_.newick_path.read_text().strip(), names)
    edges = pd.read_csv(run_.edges_path, sep="\t", float_precision="round_trip", keep_default_na=False)
    child, parent, length = want.edges()
    assert edges["child"].tolist() == child.tolist() and edges["parent"].tolist() == parent.tolist() and tc.same_bits(edges["length"].to_numpy(), length)
