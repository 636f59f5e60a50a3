"""CPU-only: the statement of the sweep (pyani_amd.screen.sweep_of_pairs) against the tests' own union-finds and scipy
(tests/screen_sweep_cases.py), the levels against the rule of candidate_pairs, and the host layers around them.  Everything is an
integer and must be EQUAL."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_components_cases as cc
from tests import screen_sweep_cases as swc


def _same_arrays(got, want, what):
    for g, w, dtype, name in zip(got, want, (np.uint64, np.uint32, np.uint32, np.uint32, np.uint64), ("entries", "components", "singletons", "largest", "pair_slots")):
        assert g.dtype == dtype, (what, name, g.dtype)
        assert g.tolist() == list(w), (what, name)


@pytest.mark.parametrize("name", sorted(set(swc.CASES) - {"big"}))
def test_statement_equals_union_find_and_scipy(name):
    from pyani_amd import screen
    a, b, s, level, n, steps, snaps = swc.CASES[name]()
    got = screen.sweep_of_pairs(a, b, level, n, steps, s, snaps)
    want, nodes = swc.expected(name)
    _same_arrays(got[:5], want, (name, "union-find"))
    _same_arrays(got[:5], swc.scipy_per_step(name), (name, "scipy"))
    assert len(got[5]) == len(snaps)
    for k, step in enumerate(snaps):
        for g, w, dtype in zip(got[5][k], nodes[step], (np.int32, np.uint64, np.uint64)):
            assert g.dtype == dtype and (g == w).all(), (name, step)


def test_statement_on_the_largest_case_equals_scipy():
    from pyani_amd import screen
    a, b, s, level, n, steps, _ = swc.big()
    _same_arrays(screen.sweep_of_pairs(a, b, level, n, steps, s)[:5], swc.scipy_per_step("big"), "big")


def _statement(name):
    from pyani_amd import screen
    a, b, s, level, n, steps, _ = swc.CASES[name]()
    return screen.sweep_of_pairs(a, b, level, n, steps, s)


def test_what_the_cases_are_for():
    assert _statement("chain_4095")[1].tolist() == list(range(1, cc.CHAIN_N))      # one component fewer per step down
    entries, _, _, _, pair_slots, _ = _statement("cliques_bridge")
    assert (pair_slots == entries).tolist() == [s >= swc.BRIDGE_LEVEL for s in range(swc.BRIDGE_STEPS)]
    a, b, _, level, _, steps, _ = swc.buckets()
    live = level[a != b]
    assert _statement("buckets")[0].tolist() == [int((live > s).sum()) for s in range(steps)]
    assert [int((level == l).sum()) for l in sorted(swc.BUCKETS)] == [swc.BUCKETS[l] for l in sorted(swc.BUCKETS)]
    for name in ("all_level_zero", "self_entries"):
        n, steps = swc.CASES[name]()[4:6]
        entries, components, _, largest, _, _ = _statement(name)
        assert entries.tolist() == [0] * steps and components.tolist() == [n] * steps and largest.tolist() == [1] * steps


@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("edges", *scr.EDGES_PARAMS)])
def test_levels_are_the_rule_of_candidate_pairs(case, k, scale):
    """level > s is, for every step, exactly the set candidate_pairs(T_s) keeps: from the numpy shared matrix, no device."""
    from pyani_amd import screen
    sizes, shared = scr.expected(case, k, scale)
    n = len(sizes)
    result = screen.ScreenResult([f"g{i}" for i in range(n)], k, scale, sizes, shared)
    need = screen.sweep_thresholds(sizes, k, swc.LADDER, 2)
    assert need.dtype == np.uint32 and need.shape == (len(swc.LADDER), n)
    for s, t in enumerate(swc.LADDER):
        assert (need[s] == screen.identity_thresholds(sizes, k, t, 2)).all()
    a, b = (x.reshape(-1) for x in np.nonzero(~np.eye(n, dtype=bool)))      # EVERY ordered pair, row-major, kept or not
    level = screen.sweep_levels(a, b, shared[a, b], need)
    assert level.dtype == np.uint16 and len(level) == len(a)
    ident = scr.identity_of(sizes, shared, k, 2)      # the tests' own restatement of the identity
    seen = set()
    for s, t in enumerate(swc.LADDER):
        got = list(zip(a[level > s].tolist(), b[level > s].tolist()))
        assert got == result.candidate_pairs(t, 2), (case, s, t)
        assert got == [(i, j) for i in range(n) for j in range(n) if i != j and (ident[i, j] >= t or ident[j, i] >= t)], (case, s, t)
        seen.add(len(got))
    assert len(seen) >= 2      # the ladder moves the set


def test_ladders_that_are_refused():
    from pyani_amd import screen
    sizes = np.array([100, 200, 50], dtype=np.uint32)
    for bad in ((0.9, 0.8), (0.8, 0.8), (0.8, float("nan")), (), np.linspace(0.5, 0.9, screen.SWEEP_MAX_STEPS + 1)):
        with pytest.raises(ValueError):
            screen.sweep_thresholds(sizes, 16, bad, 2)
    with pytest.raises(ValueError):
        screen.check_need_table(np.array([[3, 4], [3, 3]], dtype=np.uint32))      # a column falls
    with pytest.raises(ValueError):
        screen.sweep_levels([0], [1], [5], np.array([[3, 4], [2, 4]], dtype=np.uint32))
    with pytest.raises(ValueError):
        screen.sweep_of_pairs([0], [1], [3], 2, 2)      # a level above the steps
    with pytest.raises(ValueError):
        screen.sweep_of_pairs([0], [1], [1], 2, 2, snapshots=[2])
    with pytest.raises(ValueError):
        screen.sweep_of_pairs([0], [1], [1], 2, 2, snapshots=[0] * 33)
    assert screen.sweep_thresholds(sizes, 16, (0.8,), 2).shape == (1, 3)


def test_levels_of_values():
    from pyani_amd import screen
    t = (0.80, 0.90, 0.95)
    v = [float("nan"), 0.5, 0.80, 0.85, 0.90, 0.9499999, 0.95, 1.0, float("inf"), -float("inf")]
    level = screen.levels_of_values(v, t)
    assert level.dtype == np.uint16 and level.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 3, 0]
    for s, x in enumerate(t):      # present at step s iff value >= thresholds[s]
        assert ((level > s) == np.array([y >= x for y in v])).all()
    with pytest.raises(ValueError):
        screen.levels_of_values(v, (0.9, 0.8))


def _hand_made():
    """Six genomes of 1000 sampled k-mers: 0 - 1 - 2 a triangle at 0.99 / 0.99 / 0.91 identity, 3 - 4 a pair at 0.96, 5 alone."""
    from pyani_amd import screen
    k = 16
    sizes = np.full(6, 1000, dtype=np.uint32)

    def shared_for(identity):
        return int(screen.identity_thresholds([1000], k, identity, 2)[0])
    und = [(0, 1, shared_for(0.99)), (0, 2, shared_for(0.99)), (1, 2, shared_for(0.91)), (3, 4, shared_for(0.96))]
    a = np.array([x for x, y, _ in und] + [y for x, y, _ in und], dtype=np.int32)
    b = np.array([y for x, y, _ in und] + [x for x, y, _ in und], dtype=np.int32)
    s = np.array([w for _, _, w in und] * 2, dtype=np.uint32)
    order = np.lexsort((b, a))
    return screen.ScreenedPairs([f"g{i}" for i in range(6)], screen.ScreenOptions(0.90, k, 256, 2), sizes, a[order], b[order], s[order])


def test_screened_pairs_sweep_and_the_screen_sweep():
    from pyani_amd import screen
    pairs = _hand_made()
    ladder = (0.90, 0.95, 0.98, 0.995)
    sw = pairs.sweep(ladder, snapshots=(0, 2))      # engine=None: the statement
    assert isinstance(sw, screen.ScreenSweep) and sw.labels == pairs.labels and sw.identities.tolist() == list(ladder)
    assert sw.entries.tolist() == [8, 6, 4, 0] and sw.components.tolist() == [3, 3, 4, 6]
    assert sw.singletons.tolist() == [1, 1, 3, 6] and sw.largest.tolist() == [3, 3, 3, 1] and sw.pair_slots.tolist() == [8, 8, 6, 0]
    assert sw.complete.tolist() == [True, False, False, True]      # 0.95: 1 - 2 is gone, the triangle is a path
    frame = sw.frame()
    assert list(frame.columns) == ["step", "identity", "entries", "components", "singletons", "largest", "pair_slots", "complete"]
    assert len(frame) == 4 and frame["components"].tolist() == [3, 3, 4, 6] and frame["identity"].tolist() == list(ladder)
    special = sw.special()
    assert special["step"].tolist() == [0, 3] and list(special.columns) == list(frame.columns)
    at0, at2 = sw.components_at(0), sw.components_at(2)
    assert isinstance(at0, screen.ScreenComponents) and at0.size.tolist() == [3, 2, 1] and at0.complete.tolist() == [True, True, True]
    assert at0.labels == pairs.labels and at2.size.tolist() == [3, 1, 1, 1] and at2.complete.tolist() == [False, True, True, True]
    whole = pairs.components()      # the components at the pairs' own threshold are step 0's
    for f in screen.ScreenComponents._fields[1:]:
        assert (getattr(at0, f) == getattr(whole, f)).all(), f
    for step in (1, 3, 4, -1):
        with pytest.raises(IndexError):
            sw.components_at(step)
    with pytest.raises(ValueError):
        pairs.sweep((0.85, 0.95))      # below the identity the pairs were kept at
    with pytest.raises(ValueError):
        pairs.sweep(ladder, snapshots=(4,))
