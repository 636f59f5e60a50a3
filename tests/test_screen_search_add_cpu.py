"""CPU: the growth of the search index without a device — the numpy statement of the merge (pyani_amd.screen.merge_search_index:
the device's steps 3 to 5 on arrays) against a fresh grouping of random tiny sets, Engine's record of the index around an add (a stub
library), and the ValueErrors of db_batch= in both drivers, raised before a file is read or an engine is made."""
import numpy as np
import pytest


def _fresh(sets):
    """The index of a list of k-mer sets, grouped from scratch: (kmer ascending, start, member ascending inside a k-mer)."""
    holders = {}
    for g, s in enumerate(sets):
        for x in sorted(s):
            holders.setdefault(int(x), []).append(g)
    kmer = np.array(sorted(holders), dtype=np.uint32)
    counts = [len(holders[int(x)]) for x in kmer]
    member = np.array([g for x in kmer for g in holders[int(x)]], dtype=np.uint32)
    return kmer, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), member


def _entries(sets, first):
    """The added genomes' entries in the index's order: by k-mer, then genome (first + j)."""
    pairs = sorted((int(x), first + j) for j, s in enumerate(sets) for x in s)
    return np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)


def _check(old_sets, new_sets, what):
    from pyani_amd import screen
    kmer, start, member = _fresh(old_sets)
    got = screen.merge_search_index(kmer, start, member, *_entries(new_sets, len(old_sets)))
    want = _fresh(list(old_sets) + list(new_sets))
    for g, w, name in zip(got[:3], want, ("kmer", "start", "member")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g, w)
    batch = set().union(*new_sets) if new_sets else set()
    assert got[3] == len(batch - set(kmer.tolist())) and got[4] == len(batch & set(kmer.tolist())), (what, got[3:])
    return got


def test_merge_equals_a_fresh_grouping_on_random_sets():
    rng = np.random.default_rng(20261020)
    for trial in range(60):
        universe = int(rng.integers(1, 40))
        n, m = int(rng.integers(0, 6)), int(rng.integers(0, 5))
        sets = [set(rng.integers(0, universe, size=int(rng.integers(0, universe + 1))).tolist()) for _ in range(n + m)]
        _check(sets[:n], sets[n:], trial)


def test_merge_when_every_added_kmer_is_absent_and_when_none_is():
    old = [{10, 20, 30}, {20, 40}, set()]
    got = _check(old, [{5, 25}, {25, 50, 60}, {1}], "all absent")      # before the first, between, behind the last
    assert got[3:] == (5, 0)      # 1, 5, 25 (held by two of the batch), 50, 60
    got = _check(old, [{20, 40}, {10, 20, 30, 40}], "none absent")
    assert got[3:] == (0, 4) and np.array_equal(got[0], [10, 20, 30, 40])
    got = _check([set(), set()], [{7, 3}, {3}], "an index without a k-mer")
    assert got[3:] == (2, 0) and np.array_equal(got[2], [2, 3, 2])
    got = _check(old, [set(), set()], "genomes without a k-mer")
    assert got[3:] == (0, 0) and np.array_equal(got[2], _fresh(old)[2])
    _check(old, [{10, 20, 30}], "the first genome again")
    _check(old + [{10, 20, 30}], [{10, 20, 30}], "and again: two equal columns")


def test_the_engine_records_an_add_after_success_only():
    """Engine's record of the index (n, sizes, labels) grows when the library accepted the add, and stays as it was after a refusal AND
    after a later failure: the old index is still resident then (a stub library: no device)."""
    from pyani_amd import _lib
    from pyani_amd.engine import Engine

    class Lib:
        rc = 0

        def pg_screen_search_index(self, *args):
            return 0

        def pg_screen_search_index_add(self, *args):
            return self.rc

        def pg_last_error(self, h):
            return b"stub"
    e = Engine.__new__(Engine)
    e.lib, e._h = Lib(), None
    e.screen_search_index([0, 1, 2], 16, 16, labels=["a", "b", "c"])
    e._search_q = 5
    assert len(e.screen_search_index_add([])) == 0 and e._search["n"] == 3 and e._search_q == 5      # nothing added: nothing dropped
    assert len(e.screen_search_index_add([7, 8], labels=["d", "e"])) == 2
    assert e._search["n"] == 5 and e._search["labels"] == ["a", "b", "c", "d", "e"] and len(e._search["sizes"]) == 5 and e._search_q == 0
    assert (e._search["kmer"], e._search["scale"]) == (16, 16)
    assert e.screen_search_index_add([3]) is not None and e._search["labels"][-1] == "3"      # default labels: the ids
    for rc in (_lib.PG_E_ARG, _lib.PG_E_NOMEM):
        e.lib.rc = rc
        with pytest.raises(_lib.PyaniGpuError):
            e.screen_search_index_add([9])
        assert e._search["n"] == 6 and len(e._search["labels"]) == 6
    with pytest.raises(ValueError, match="same length"):
        e.screen_search_index_add([1, 2], labels=["x"])


class NoEngine:      # any use would raise AttributeError, not ValueError
    pass


def _drivers():
    from pyani_amd.subcmd_gather import run_screen_gather
    from pyani_amd.subcmd_search import run_screen_search
    return ((run_screen_search, {"min_identity": 0.8}), (run_screen_gather, {"min_unique": 5}))


def test_db_batch_refusals_come_before_any_engine(tmp_path, monkeypatch):
    from pyani_amd import subcmd_gather, subcmd_search

    def no_engine(*a, **kw):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(subcmd_search, "default_engine", no_engine)
    monkeypatch.setattr(subcmd_gather, "default_engine", no_engine)
    missing = tmp_path / "does_not_exist"
    for run, args in _drivers():
        for bad in (0, -1, 1.5, True, False, "2", [2]):
            with pytest.raises(ValueError, match="db_batch must be an integer >= 1"):
                run(missing, missing, db_batch=bad, **args)
        with pytest.raises(ValueError, match="exact="):
            run(missing, missing, db_batch=2, exact="anim", **args)
        with pytest.raises(ValueError, match="single Engine"):
            run(missing, missing, db_batch=2, engine=NoEngine(), **args)
    with pytest.raises(ValueError, match="single Engine"):
        subcmd_search.run_screen_search(missing, missing, min_identity=0.8, db_batch=2, devices=[0, 1])
    with pytest.raises(ValueError, match="single Engine"):
        subcmd_search.run_screen_search(missing, missing, min_identity=0.8, db_batch=2, workers=2)


def test_db_batch_needs_an_empty_store(tmp_path):
    """The store is looked at before a file is read: a stub that is an Engine without a device and holds a genome."""
    from pyani_amd.engine import Engine

    class Holding(Engine):
        def __init__(self):      # no library, no device
            pass

        def genome_count(self):
            return 1

        def __del__(self):
            pass
    missing = tmp_path / "does_not_exist"
    for run, args in _drivers():
        with pytest.raises(ValueError, match="store is empty"):
            run(missing, missing, db_batch=2, engine=Holding(), **args)
        with pytest.raises(ValueError, match="exact="):
            run(missing, missing, db_batch=2, exact="anim", engine=Holding(), **args)
