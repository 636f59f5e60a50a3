"""The inputs of the sweep's tests (tests/test_screen_sweep_cpu.py, tests/test_screen_sweep_gpu.py), built on the lists of
tests/screen_components_cases.py with deterministic levels, and references that share nothing with pyani_amd/screen.py: the union-find
of that file run afresh per step, a nested union-find written here that takes the levels in from the top, and
scipy.sparse.csgraph.connected_components run afresh per step.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.

A case is (a int32[m], b int32[m], shared uint32[m] or None, level uint16[m], n, steps, snapshots).  Entry e is present at step s iff
level[e] > s.  Everything expected is an integer and must be EQUAL."""
import functools

import numpy as np

from tests import screen_components_cases as cc


def _case(a, b, shared, level, n, steps, snapshots=None):
    a, b, s, n = cc._case(a, b, shared, n)
    level = np.ascontiguousarray(level, dtype=np.uint16)
    assert len(level) == len(a) and (not len(level) or int(level.max()) <= steps)
    level.setflags(write=False)
    if snapshots is None:
        snapshots = sorted({0, steps // 2, steps - 1})
    return a, b, s, level, n, int(steps), tuple(int(x) for x in snapshots)


def one_node():
    """n = 1, m = 0, S = 1."""
    return _case([], [], [], [], 1, 1)


def self_entries():
    """Self entries only, at levels 1, 2, 3 and 0: nothing is counted at any step."""
    a, b, s, n = cc.self_entries()
    return _case(a, b, s, [1, 2, 3, 0], n, 3)


def _small_graph():
    rng = np.random.default_rng(51)
    u, v = rng.integers(0, 400, 700), rng.integers(0, 400, 700)
    a, b, s = cc._both_ways(u, v, rng, rng.integers(1, 900, 700))
    return a, b, s, 400


def all_level_zero():
    """Every entry at level 0: present at no step, n singletons everywhere, no bucket."""
    a, b, s, n = _small_graph()
    return _case(a, b, s, np.zeros(len(a)), n, 4)


def all_level_top():
    """Every entry at level S: ONE bucket, every lower step copies its row."""
    a, b, s, n = _small_graph()
    return _case(a, b, s, np.full(len(a), 4), n, 4)


def chain_64():
    """The shuffled chain of 4096 with S = 64, link u at level 1 + u mod 64: every bucket joins trees the earlier buckets left."""
    a, b, s, n = cc.chain("shuffled")
    return _case(a, b, s, 1 + a % 64, n, 64)


CHAIN_STEPS = cc.CHAIN_N - 1


def chain_4095():
    """The chain of 4096 with S = 4095, ONE link per level: the components fall by exactly one per step, and it is the most launches."""
    a, b, s, n = cc.chain("ascending")
    return _case(a, b, s, 1 + a, n, CHAIN_STEPS)


BRIDGE_STEPS, BRIDGE_LEVEL = 8, 3


def cliques_bridge():
    """Two cliques of 300, both directions, at level S, and ONE bridge entry at level 3, shuffled: complete for s >= 3, not below."""
    a, b, s, n = cc.cliques(True, True)
    bridge = ((a == 0) & (b == cc.CLIQUE)) | ((a == cc.CLIQUE) & (b == 0))
    assert int(bridge.sum()) == 1
    return _case(a, b, s, np.where(bridge, BRIDGE_LEVEL, BRIDGE_STEPS), n, BRIDGE_STEPS, snapshots=(0, BRIDGE_LEVEL - 1, BRIDGE_LEVEL, BRIDGE_STEPS - 1))


BUCKETS = {7: 0, 6: 63, 5: 64, 4: 0, 3: 65, 2: 10, 1: 0, 0: 5}      # level -> entries: empty buckets at both ends and in the middle


def buckets():
    """Buckets of 63, 64 and 65 entries (one wave less one, one wave, one wave and one) with empty buckets at the top, the bottom and in
    the middle (their rows are copied), and five entries of level 0."""
    rng = np.random.default_rng(52)
    m = sum(BUCKETS.values())
    level = rng.permutation(np.concatenate([np.full(c, l) for l, c in BUCKETS.items()]))
    return _case(rng.integers(0, 150, m), rng.integers(0, 150, m), rng.integers(1, 50, m), level, 150, 7, snapshots=(0, 1, 3, 4, 6))


def one_direction_duplicates():
    """Entries in one direction only, some given twice at DIFFERENT levels: the copies enter at their own steps, the second joins nothing."""
    a = [1, 1, 2, 2, 4, 4, 3]
    b = [0, 0, 1, 1, 3, 3, 4]
    return _case(a, b, [5, 6, 7, 8, 9, 10, 11], [2, 1, 3, 3, 1, 2, 3], 6, 3, snapshots=(0, 1, 2))


STAR_STEPS = 16


def star():
    """The star of 70 000 leaves with leaf i at level 1 + i mod 16: contention on ONE tree in every bucket."""
    a, b, s, n = cc.star()
    return _case(a, b, s, 1 + b % STAR_STEPS, n, STAR_STEPS)


def unweighted():
    """shared=None: every entry weighs 1."""
    a, b, _, n = cc.unweighted()
    return _case(a, b, None, (a + b) % 6, n, 5)


BIG_N, BIG_ENTRIES, BIG_STEPS = cc.MAX_N, 2_000_000, 8


@functools.lru_cache(maxsize=None)
def big():
    """n = 2^20 with 2 x 10^6 random entries (one direction, duplicates and self entries as they fall) and S = 8, levels 0 ... 8."""
    rng = np.random.default_rng(53)
    return _case(rng.integers(0, BIG_N, BIG_ENTRIES), rng.integers(0, BIG_N, BIG_ENTRIES), rng.integers(1, 1000, BIG_ENTRIES),
                 rng.integers(0, BIG_STEPS + 1, BIG_ENTRIES), BIG_N, BIG_STEPS)


CASES = {
    "one_node": one_node, "self_entries": self_entries, "all_level_zero": all_level_zero, "all_level_top": all_level_top, "chain_64": chain_64,
    "chain_4095": chain_4095, "cliques_bridge": cliques_bridge, "buckets": buckets, "one_direction_duplicates": one_direction_duplicates,
    "star": star, "unweighted": unweighted, "big": big,
}

LADDER = (0.80, 0.85, 0.90, 0.95, 0.99)      # the index form's and sweep_levels' tests


# ---- the references ------------------------------------------------------------------------------------------------------------------------------
def _row_of_roots(root, n):
    size = np.bincount(root, minlength=n)
    size = size[size > 0].astype(object)      # (Python integers: no width to overflow)
    return len(size), int((size == 1).sum()), int(size.max()), int((size * (size - 1)).sum())


def per_step(case, roots_of):
    """The five per-step arrays of a case as Python integers, from roots_of(a, b, n) -> root run afresh on the entries present at each
    step."""
    a, b, s, level, n, steps, _ = case
    rows = []
    for step in range(steps):
        here = level > step
        rows.append((int((a[here] != b[here]).sum()),) + _row_of_roots(roots_of(a[here], b[here], n), n))
    return [list(col) for col in zip(*rows)]      # entries, components, singletons, largest, pair_slots


def nested_union_find(case):
    """The five per-step arrays by ONE sequential union-find in Python integers that takes the levels in from the top: the sizes of the
    trees are kept at their roots, and every union updates the four figures.  Its own code, no numpy in the loop."""
    a, b, _, level, n, steps, _ = case
    parent, size = list(range(n)), [1] * n

    def find(x):
        top = x
        while parent[top] != top:
            top = parent[top]
        while parent[x] != top:
            parent[x], x = top, parent[x]
        return top
    order = np.argsort(-level.astype(np.int64), kind="stable")
    al, bl, ll = a[order].tolist(), b[order].tolist(), level[order].tolist()
    rows = [None] * steps
    present, comps, single, slots, at = 0, n, n, 0, 0
    sizes_seen = {1: n}      # size -> trees of that size
    for step in range(steps - 1, -1, -1):
        while at < len(ll) and ll[at] == step + 1:
            x, y = al[at], bl[at]
            at += 1
            if x == y:
                continue
            present += 1
            rx, ry = find(x), find(y)
            if rx == ry:
                continue
            sx, sy = size[rx], size[ry]
            for z in (sx, sy):
                sizes_seen[z] -= 1
                if not sizes_seen[z]:
                    del sizes_seen[z]
            sizes_seen[sx + sy] = sizes_seen.get(sx + sy, 0) + 1
            comps -= 1
            single -= (sx == 1) + (sy == 1)
            slots += (sx + sy) * (sx + sy - 1) - sx * (sx - 1) - sy * (sy - 1)
            parent[max(rx, ry)] = min(rx, ry)
            size[min(rx, ry)] = sx + sy
        rows[step] = (present, comps, single, max(sizes_seen), slots)
    return [list(col) for col in zip(*rows)]


UNION_FIND_STEPS = 64      # cc.union_find run afresh per step costs n Python steps a run: at every step up to here, at the snapshots beyond


@functools.lru_cache(maxsize=None)
def expected(name):
    """(per-step arrays, {snapshot step: (root, entries, weight)}) of a case by the tests' own union-finds: the arrays by
    nested_union_find — and by cc.union_find run afresh at every step where there are at most 64 steps, asserted equal here — and the
    node arrays by cc.union_find on the entries present at the snapshot.  Computed once, shared, read-only.  `big` has neither: a Python
    loop over 2^20 nodes per step is minutes; scipy_per_step holds its arrays."""
    assert name != "big"
    case = CASES[name]()
    a, b, s, level, n, steps, snaps = case
    arrays = nested_union_find(case)
    if steps <= UNION_FIND_STEPS:
        assert arrays == per_step(case, lambda x, y, n_: cc.union_find(x, y, None, n_)[0]), name
    nodes = {}
    for step in snaps:
        here = level > step
        nodes[step] = cc.union_find(a[here], b[here], None if s is None else s[here], n)
        for x in nodes[step]:
            x.setflags(write=False)
    return arrays, nodes


@functools.lru_cache(maxsize=None)
def scipy_per_step(name):
    """The five per-step arrays with scipy.sparse.csgraph.connected_components run afresh on the entries present at each step."""
    return per_step(CASES[name](), lambda x, y, n_: cc.scipy_roots(x, y, n_)[0])
