"""CPU: the integer form of the screen's selection rule (pyani_amd.screen.identity_thresholds).  The numpy statement of
the rule (tests/screen_select_cases.rule) must equal ScreenResult.candidate_pairs — the float rule it replaces — in content and in
order, on the screen's own test cases and on random matrices; identity_thresholds must equal a scan over every count."""
import itertools

import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_select_cases as ssc


def _result(sizes, shared, k):
    from pyani_amd.screen import ScreenResult
    return ScreenResult([f"g{i}" for i in range(len(sizes))], k, 16, np.asarray(sizes, dtype=np.uint32), np.asarray(shared, dtype=np.uint32))


def _check_matrix(sizes, shared, what, min_shareds=(2,)):
    from pyani_amd.screen import identity_thresholds
    n = len(sizes)
    some, fewer = False, False
    for k in ssc.KMERS:
        res = _result(sizes, shared, k)
        for ms in min_shareds:
            for t in ssc.THRESHOLDS:
                want = res.candidate_pairs(t, ms)
                a, b, s = ssc.rule(shared, identity_thresholds(sizes, k, t, ms))
                w = np.fromiter(itertools.chain.from_iterable(want), dtype=np.int64, count=2 * len(want)).reshape(-1, 2)      # (lists of up to 9 x 10^6 pairs)
                assert len(a) == len(want) and (a == w[:, 0]).all() and (b == w[:, 1]).all(), (what, k, ms, t, len(a), len(want))
                assert (s == np.asarray(shared)[a, b]).all()
                some |= len(want) > 0
                fewer |= len(want) < n * (n - 1)
    assert some and fewer, what


@pytest.mark.parametrize("case,k,scale", [("family", 16, 16), ("family", 12, 16), ("edges", *scr.EDGES_PARAMS), ("wide", *scr.WIDE_PARAMS)])
def test_integer_rule_equals_candidate_pairs_on_the_screen_cases(case, k, scale):
    """(The wide case takes most of a minute: every genome of it shares one motif, so candidate_pairs itself builds a list of 9 x 10^6
    tuples for most of its eighteen (k, threshold) combinations; the rule's side is a fraction of a second each.)"""
    sizes, shared = scr.expected(case, k, scale)
    _check_matrix(sizes, shared, (case, k, scale), min_shareds=(2,) if case == "wide" else (1, 2, 5))


@pytest.mark.parametrize("seed,n", [(1, 2), (2, 17), (3, 100), (4, 300)])
def test_integer_rule_equals_candidate_pairs_on_random_matrices(seed, n):
    sizes, shared = ssc.random_symmetric(seed, n)
    assert sizes.max() <= 5000 and (shared == shared.T).all() and (shared <= np.minimum.outer(sizes, sizes)).all()
    _check_matrix(sizes, shared, ("random", seed, n), min_shareds=(1, 2, 9))


def test_thresholds_equal_a_scan_over_every_count():
    from pyani_amd.screen import identity_thresholds
    top = 2000
    size = np.arange(1, top + 1)
    s = np.arange(0, top + 1)
    thresholds = ssc.THRESHOLDS + (0.25, 0.95, 0.99, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 2.0)
    for k in ssc.KMERS:
        with np.errstate(all="ignore"):
            ident = np.power(s[None, :].astype(np.float64) / size[:, None].astype(np.float64), 1.0 / k)      # [size, s]; s > size unused
        inside = s[None, :] <= size[:, None]
        for ms in (1, 2, 7, 1999, 2001):
            for t in thresholds:
                ok = inside & (s[None, :] >= ms) & (ident >= t)
                want = np.where(ok.any(axis=1), ok.argmax(axis=1), size + 1)
                if t <= 0:
                    want = np.zeros(top, dtype=np.int64)
                got = identity_thresholds(size, k, t, ms)
                assert got.dtype == np.uint32 and (got == want).all(), (k, ms, t, np.flatnonzero(got != want)[:5])


def test_threshold_edge_cases():
    from pyani_amd.screen import identity_thresholds
    sizes = np.array([0, 1, 5, 100, 4097], dtype=np.uint32)
    assert identity_thresholds(sizes, 16, 0.0).tolist() == [0] * 5 and identity_thresholds(sizes, 16, -1.0, 3).tolist() == [0] * 5
    assert identity_thresholds(sizes, 16, 1.0).tolist() == [1, 2, 5, 100, 4097]      # only a full row reaches 1.0; sizes 0 and 1 have no s >= 2
    assert identity_thresholds(sizes, 16, 1.0, 1).tolist() == [1, 1, 5, 100, 4097]
    assert identity_thresholds(sizes, 16, 1.5).tolist() == [1, 2, 6, 101, 4098]      # nothing reaches it: size + 1
    assert identity_thresholds(sizes, 16, 0.5, 6).tolist() == [1, 2, 6, 6, 6]        # min_shared above the size: size + 1; else the floor decides
    assert identity_thresholds(sizes, 8, 1e-300, 2).tolist() == [1, 2, 2, 2, 2]      # any positive threshold: the floor
    assert identity_thresholds([], 16, 0.8).shape == (0,)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            identity_thresholds(sizes, 16, 0.8, bad)
    with pytest.raises(ValueError):
        identity_thresholds(sizes, 7, 0.8)
    with pytest.raises(ValueError):
        identity_thresholds(sizes, 16, float("nan"))


def test_options_validation():
    from pyani_amd.screen import ScreenOptions, check_options
    assert ScreenOptions(0.8) == (0.8, 16, 256, 2)
    assert check_options(0.8) == ScreenOptions(0.8, 16, 256, 2) and check_options(0) == ScreenOptions(0.0, 16, 256, 2)
    assert check_options(ScreenOptions(0.9, kmer=12, scale=16, min_shared=1)) == ScreenOptions(0.9, 12, 16, 1)
    assert isinstance(check_options(np.float64(0.5)).min_identity, float)
    for bad in (ScreenOptions(0.8, kmer=7), ScreenOptions(0.8, kmer=17), ScreenOptions(0.8, scale=3), ScreenOptions(0.8, scale=131072),
                ScreenOptions(0.8, min_shared=0), ScreenOptions(0.8, min_shared=1.5), ScreenOptions(float("nan")), ScreenOptions("0.8"), "0.8",
                None, True, (0.8, 16)):
        with pytest.raises(ValueError):
            check_options(bad)


def test_screened_pairs_arithmetic():
    from pyani_amd.screen import ScreenOptions, ScreenedPairs
    sp = ScreenedPairs(["x", "y", "z"], ScreenOptions(0.0, 16, 16, 2), np.array([100, 50, 0], dtype=np.uint32), np.array([0, 1, 2, 0], dtype=np.int32),
                       np.array([1, 0, 0, 2], dtype=np.int32), np.array([25, 25, 0, 1], dtype=np.uint32))
    assert sp.pairs() == [(0, 1), (1, 0), (2, 0), (0, 2)]
    c, i = sp.containment(), sp.identity()
    assert c[0] == 0.25 and c[1] == 0.5 and np.isnan(c[2]) and c[3] == 0.01
    assert i[0] == np.power(0.25, 1 / 16) and i[1] == np.power(0.5, 1 / 16) and i[2] == 0.0 and i[3] == 0.0      # below the floor: 0.0
    f = sp.frame()
    assert list(f.columns) == ["query", "subject", "shared", "containment", "identity"] and list(f["query"]) == ["x", "y", "z", "x"]


def test_drivers_refuse_before_any_work():
    from pyani_amd.screen import ScreenOptions
    from pyani_amd.subcmd_anib import run_anib
    from pyani_amd.subcmd_anim import run_anim
    for run in (run_anim, run_anib):
        with pytest.raises(ValueError):
            run("nowhere", screen=ScreenOptions(0.8, min_shared=0))
        with pytest.raises(ValueError):
            run("nowhere", screen="0.8")
    for kw in (dict(distributed=True), dict(group=object())):
        with pytest.raises(ValueError, match="collective"):
            run_anim("nowhere", screen=0.8, **kw)


def test_header_bindings_and_library_agree_on_the_selection_calls():
    import re
    from pyani_amd import _lib, build
    from tests.conftest import ROOT
    build.build_gpu()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    for sym, arity in (("pg_screen_hold", 8), ("pg_screen_load", 3), ("pg_screen_select", 4), ("pg_screen_select_read", 4), ("pg_screen_fetch", 2),
                       ("pg_screen_release", 1)):
        m = re.search(rf"\bint {sym}\s*\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[sym][1]) and hasattr(lib, sym), sym


def test_the_run_genomes_split_into_two_families_on_the_statement():
    """The design the GPU run test relies on, from the numpy statement of the screen alone: ScreenOptions(0.8, scale=16) keeps exactly the
    12 within-family ordered pairs of the six genomes and drops the other 18."""
    from pyani_amd.screen import identity_thresholds
    sizes, shared = scr.statement(ssc.run_genomes(), 16, 16)
    a, b, _ = ssc.rule(shared, identity_thresholds(sizes, 16, 0.8, 2))
    kept = [(ssc.RUN_STEMS[x], ssc.RUN_STEMS[y]) for x, y in zip(a, b)]
    assert kept == ssc.RUN_KEPT and len(kept) == 12
    assert _result(sizes, shared, 16).candidate_pairs(0.8) == list(zip(a.tolist(), b.tolist()))
