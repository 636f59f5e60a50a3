"""The inputs of the representatives' tests (tests/test_screen_representatives_cpu.py, tests/test_screen_representatives_gpu.py): the lists
of tests/screen_components_cases.py under four kinds of scores, and a reference that shares nothing with pyani_amd/screen.py: the
sequential greedy walk, written here in Python dicts.  TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.

Everything expected is an integer and must be EQUAL."""
import functools
import random

import numpy as np

from tests import fuzz_genomes
from tests import screen_components_cases as cc

SCORE_KINDS = ("index", "reversed", "random", "constant")


def scores(kind, n):
    """uint64[n]: `index` n - 1 - v (node 0 is best), `reversed` v (node n - 1 is best), `random` seeded 40-bit values (ties are rare but
    exist beyond 2^20 draws), `constant` (every tie goes to the smaller index)."""
    if kind == "index":
        s = np.arange(n, dtype=np.uint64)[::-1].copy()
    elif kind == "reversed":
        s = np.arange(n, dtype=np.uint64)
    elif kind == "random":
        s = np.random.default_rng(n + 7).integers(0, 1 << 40, n).astype(np.uint64)
    elif kind == "constant":
        s = np.full(n, 5, dtype=np.uint64)
    else:
        raise KeyError(kind)
    s.setflags(write=False)
    return s


# the kinds every case runs under: all four for the small lists, two each for the two big ones (the walk is Python)
def kinds_of(name):
    return {"star": ("index", "reversed"), "largest": ("reversed", "random")}.get(name, SCORE_KINDS)


PAIRS = [(name, kind) for name in sorted(cc.CASES) for kind in kinds_of(name)]


def neighbours(a, b, weight):
    """{v: {u: pair weight}}: direction ignored, self-entries dropped, the maximum over the entries of a pair."""
    nbr = {}
    ws = [1] * len(a) if weight is None else weight.tolist()
    for x, y, w in zip(a.tolist(), b.tolist(), ws):
        if x == y:
            continue
        for p, q in ((x, y), (y, x)):
            d = nbr.setdefault(p, {})
            if d.get(q, -1) < w:
                d[q] = w
    return nbr


def walk(a, b, weight, n, score, assign_during_walk=False):
    """(rep int32[n], via uint32[n]) by the sequential greedy rule in Python integers.  assign_during_walk: CD-HIT's variant, every
    node joining the best representative known when the walk reaches it — NOT the rule of the feature; the tests show the two differ."""
    nbr = neighbours(a, b, weight)
    sc = score.tolist()
    order = sorted(range(n), key=lambda v: (-sc[v], v))
    rank = {v: i for i, v in enumerate(order)}
    reps = set()
    rep, via = list(range(n)), [0] * n

    def best_of(v):
        w, minus_rank, r = max((w, -rank[r], r) for r, w in nbr[v].items() if r in reps)
        return r, w
    for v in order:
        if any(u in reps for u in nbr.get(v, ())):
            if assign_during_walk:
                rep[v], via[v] = best_of(v)
        else:
            reps.add(v)
    if not assign_during_walk:
        for v in range(n):
            if v not in reps:
                rep[v], via[v] = best_of(v)
    return np.array(rep, dtype=np.int32), np.array(via, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def expected(name, kind):
    """(rep, via) of a case under a kind of scores by the tests' walk: computed once, shared, read-only."""
    a, b, s, n = cc.CASES[name]()
    out = walk(a, b, s, n, scores(kind, n))
    for x in out:
        x.setflags(write=False)
    return out


def after_the_walk():
    """A path r1 - v - r2 with rank(r1) < rank(v) < rank(r2): r1 covers v, so r2 becomes a representative too, and r2 holds the greater
    weight.  The rule gives v to r2; assigning during the walk would give it to r1."""
    a, b, w = np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([3, 9], np.uint32)
    return a, b, w, 3, np.array([10, 5, 1], dtype=np.uint64)


# ---- run_dereplicate's genomes ------------------------------------------------------------------------------------------------------------
FAMILIES, PER_FAMILY, FAMILY_BASES = 3, 4, 30_000


def family_genomes():
    """{stem: sequence}: three unrelated random ancestors of 30 kb, four descendants each (tests/fuzz_genomes.mutate: 0.8 % substitutions
    and 0.1 % indels against the ancestor, so two of a family differ by less than 2 %), named f<family>g<k>."""
    rng = random.Random(20261020)
    out = {}
    for f in range(FAMILIES):
        ancestor = "".join(rng.choice("ACGT") for _ in range(FAMILY_BASES))
        for k in range(PER_FAMILY):
            out[f"f{f}g{k}"] = fuzz_genomes.mutate(rng, ancestor, 0.008, 0.001)
    return out


def family_scores():
    """{stem: score}: the best of family f is genome (f + 1) % 4 — never the first of its family in sorted order for all three."""
    return {f"f{f}g{k}": (100.0 if k == (f + 1) % PER_FAMILY else 10.0 + k) for f in range(FAMILIES) for k in range(PER_FAMILY)}
