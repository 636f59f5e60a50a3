"""CPU: the search index on disk and its shrinking without a device — the numpy statement of the remove
(pyani_amd.screen.remove_from_search_index) against a fresh grouping of random tiny sets, alone and interleaved with the merge; the
file's round trip and every refusal of its reader; the numpy statement of the import's validation (check_search_index) on a built index
and on single corruptions; Engine's record of the index around a load and a remove (a stub library); and the ValueErrors of index= in
both drivers and of the database drivers, raised before a file is read or an engine is made."""
import os

import numpy as np
import pytest

from tests import screen_store_cases as stc
from tests.test_screen_search_add_cpu import _entries, _fresh


def _same(got, want, what):
    for g, w, name in zip(got, want, ("kmer", "start", "member")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g, w)


def _check(sets, columns, what):
    from pyani_amd import screen
    kmer, start, member = _fresh(sets)
    got = screen.remove_from_search_index(kmer, start, member, len(sets), columns)
    left = [s for g, s in enumerate(sets) if g not in set(columns)]
    want = _fresh(left)
    _same(got[:3], want, what)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int64 and got[2].dtype == np.uint32
    assert got[3] == sum(len(sets[c]) for c in columns), (what, got[3])
    assert got[4] == len(kmer) - len(want[0]), (what, got[4])
    return got


def test_remove_equals_a_fresh_grouping_on_random_sets():
    rng = np.random.default_rng(20261021)
    for trial in range(60):
        universe = int(rng.integers(1, 40))
        n = int(rng.integers(0, 8))
        sets = [set(rng.integers(0, universe, size=int(rng.integers(0, universe + 1))).tolist()) for _ in range(n)]
        m = int(rng.integers(0, n + 1))
        _check(sets, rng.permutation(n)[:m].tolist(), trial)


def test_remove_directed_cases():
    sets = [{10, 20, 30}, {20, 40}, set(), {10, 20, 30}, {50}, {20, 60, 70}]
    got = _check(sets, [], "none removed")
    assert got[3:] == (0, 0) and np.array_equal(got[2], _fresh(sets)[2])
    got = _check(sets, list(range(6)), "all removed")
    assert len(got[0]) == 0 and np.array_equal(got[1], [0]) and len(got[2]) == 0 and got[3:] == (12, 7)
    _check(sets, [0], "the first column")
    _check(sets, [5], "the last column")
    got = _check(sets, [4, 5], "the only holder of singleton k-mers")
    assert got[4] == 3      # 50, 60 and 70 go with their holders
    got = _check(sets, [3], "one of two equal columns")
    assert got[4] == 0 and np.array_equal(got[0], _fresh(sets)[0])
    got = _check(sets, [2], "a genome without a k-mer")
    assert got[3:] == (0, 0)
    _check([set(), set()], [1], "an index without a k-mer")
    _check([set(), set()], [0, 1], "an index without a k-mer, emptied")
    _check(sets, [5, 0, 3], "columns in any order")


def test_remove_refuses_bad_columns():
    from pyani_amd import screen
    kmer, start, member = _fresh([{1}, {2}])
    for bad, word in (([2], "not in an index"), ([-1], "not in an index"), ([0, 0], "twice")):
        with pytest.raises(ValueError, match=word):
            screen.remove_from_search_index(kmer, start, member, 2, bad)


def test_merge_then_remove_and_remove_then_merge():
    from pyani_amd import screen
    rng = np.random.default_rng(77)
    for trial in range(20):
        universe = int(rng.integers(2, 30))
        sets = [set(rng.integers(0, universe, size=int(rng.integers(0, universe + 1))).tolist()) for _ in range(7)]
        old, new = sets[:4], sets[4:]
        gone = rng.permutation(7)[:int(rng.integers(0, 7))].tolist()
        merged = screen.merge_search_index(*_fresh(old), *_entries(new, 4))[:3]
        got = screen.remove_from_search_index(*merged, 7, gone)[:3]
        _same(got, _fresh([s for g, s in enumerate(sets) if g not in gone]), (trial, "merge, remove"))
        gone_old = [g for g in gone if g < 4]
        left = [s for g, s in enumerate(old) if g not in gone_old]
        shrunk = screen.remove_from_search_index(*_fresh(old), 4, gone_old)[:3]
        got = screen.merge_search_index(*shrunk, *_entries(new, len(left)))[:3]
        _same(got, _fresh(left + new), (trial, "remove, merge"))


# ---- the file --------------------------------------------------------------------------------------------------------------------------------
def _file_args(index):
    shape, arrays = index
    n = shape[0]
    from pyani_amd import screen
    return shape, arrays, screen.search_index_sizes(arrays[2], n), [f"genome {g}" for g in range(n)], np.arange(n, dtype=np.uint64) * 1000 + 7


def _round_trip(tmp_path, index, name):
    from pyani_amd import screen
    shape, arrays, sizes, labels, lengths = _file_args(index)
    path = tmp_path / name
    size = screen.write_search_index(path, shape, arrays, sizes, labels, lengths)
    assert os.path.getsize(path) == size and not os.path.exists(str(path) + ".tmp")
    f = screen.read_search_index(path)
    assert f.shape == tuple(shape) and f.labels == labels
    for got, want in zip(f.arrays + (f.sizes, f.lengths), tuple(arrays) + (sizes, lengths)):
        assert got.dtype == np.asarray(want).dtype and np.array_equal(got, want)
    return path, f


def test_the_file_round_trip(tmp_path):
    from pyani_amd import screen
    built = stc.built_index()
    path, f = _round_trip(tmp_path, built, "built.idx")
    assert isinstance(f.arrays[2], np.memmap) and not f.arrays[2].flags.writeable
    assert screen.check_search_index(f.shape, *f.arrays) == []
    for name, dtype, count, at in screen._search_file_layout(*(f.shape[i] for i in (0, 3, 4, 5)), 1)[0]:
        assert at % 64 == 0, name
    no_kmer = ((3, 16, 16, 0, 0, 0, 0), (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64),
                                         np.full(4096, 0xFFFFFFFF, np.uint32)))
    _round_trip(tmp_path, no_kmer, "no_kmer.idx")
    _, f = _round_trip(tmp_path, ((0,) + no_kmer[0][1:], no_kmer[1]), "no_genome.idx")
    assert f.labels == [] and len(f.sizes) == 0
    # lengths=None: zeros
    shape, arrays, sizes, labels, _ = _file_args(built)
    screen.write_search_index(tmp_path / "z.idx", shape, arrays, sizes, labels, None)
    assert not screen.read_search_index(tmp_path / "z.idx").lengths.any()


def test_every_refusal_of_the_reader(tmp_path):
    from pyani_amd import screen
    path, _ = _round_trip(tmp_path, stc.built_index(), "good.idx")
    good = path.read_bytes()
    head = screen._SEARCH_HEADER

    def refused(data, word):
        bad = tmp_path / "bad.idx"
        bad.write_bytes(data)
        with pytest.raises(ValueError, match=word):
            screen.read_search_index(bad)

    def with_field(name, value):
        h = np.frombuffer(good[:head.itemsize], dtype=head).copy()
        h[name] = value
        return h.tobytes() + good[head.itemsize:]

    refused(b"NOTANIDX" + good[8:], "wrong magic")
    refused(with_field("version", 2), "version 2")
    refused(with_field("n_bins", 2048), "N_BINS")
    refused(with_field("probe", 12345), "probe word")
    refused(good[:-1], "shorter")
    refused(good + b"\0", "longer")
    refused(good[:10], "too few")
    refused(with_field("E", int(np.frombuffer(good[:head.itemsize], dtype=head)["E"][0]) + 100), "shorter")
    # a label count other than n: the labels' bytes stay, one separator becomes a letter
    labels_at = len(good) - int(np.frombuffer(good[:head.itemsize], dtype=head)["label_bytes"][0])
    cut = good.index(b"\n", labels_at)
    refused(good[:cut] + b"x" + good[cut + 1:], "labels for")


def test_a_failed_write_leaves_no_file(tmp_path):
    from pyani_amd import screen
    shape, arrays, sizes, labels, lengths = _file_args(stc.built_index())
    path = tmp_path / "never.idx"
    with pytest.raises(ValueError, match="newline"):
        screen.write_search_index(path, shape, arrays, sizes, ["a\nb"] + labels[1:], lengths)
    with pytest.raises(ValueError, match="labels for"):
        screen.write_search_index(path, shape, arrays, sizes, labels[1:], lengths)
    with pytest.raises(ValueError, match="elements where the shape gives"):
        screen.write_search_index(path, shape, (arrays[0], arrays[1], arrays[2][:-1], arrays[3], arrays[4]), sizes, labels, lengths)

    class Breaks:      # an array that fails while it is written: the file is open by then
        def __len__(self):
            return len(arrays[2])

        def __array__(self, *a, **kw):
            raise OSError("the disk is full")
    with pytest.raises(OSError, match="disk is full"):
        screen.write_search_index(path, shape, (arrays[0], arrays[1], Breaks(), arrays[3], arrays[4]), sizes, labels, lengths)
    assert not path.exists() and not os.path.exists(str(path) + ".tmp")
    # an earlier good file stays when a later write to the same path fails
    screen.write_search_index(path, shape, arrays, sizes, labels, lengths)
    before = path.read_bytes()
    with pytest.raises(OSError):
        screen.write_search_index(path, shape, (arrays[0], arrays[1], Breaks(), arrays[3], arrays[4]), sizes, labels, lengths)
    assert path.read_bytes() == before and not os.path.exists(str(path) + ".tmp")


# ---- the validation's statement ------------------------------------------------------------------------------------------------------------
def test_the_numpy_hash_is_the_definitions():
    from pyani_amd import screen
    x = np.random.default_rng(5).integers(0, 2 ** 32, size=5000, dtype=np.uint64)
    for scale in (1, 4, 256, 65536):
        assert np.array_equal(screen.kmer_bin(x.astype(np.uint32), scale), stc.bin_of(x, scale))
        assert np.array_equal(screen.kmer_sampled(x.astype(np.uint32), scale), (stc.mix(x) & np.uint64(scale - 1)) == 0)
    assert screen.search_file_probe() == int(stc.mix([screen.SEARCH_FILE_PROBE_INPUT])[0])
    assert int(screen.mix32([1])[0]) == 0x514E28B7      # murmur3's finaliser of 1


def test_check_accepts_a_built_index_and_names_each_corruption():
    from pyani_amd import screen
    shape, arrays = stc.built_index()
    assert screen.check_search_index(shape, *arrays) == []
    shape3, arrays3 = stc.three_slices()
    assert screen.check_search_index(shape3, *arrays3) == []
    inv = screen.SEARCH_INDEX_INVARIANTS
    seen = set()
    for name, (bad_shape, bad_arrays, invariant) in stc.corruptions().items():
        got = screen.check_search_index(bad_shape, *bad_arrays)
        assert got and got[0].startswith(inv[invariant]), (name, got)
        seen.add(invariant)
    assert seen >= {"member_range", "member_order", "kmer_order", "kmer_slice", "kmer_sampled", "start_order", "start_end", "start0", "kmer_range",
                    "slice_first", "bin_slice", "shape"}


# ---- Engine's record -------------------------------------------------------------------------------------------------------------------------
def _stub_engine():
    from pyani_amd.engine import Engine

    class Lib:
        rc = 0
        sizes = None

        def pg_screen_search_index(self, *args):
            return 0

        def pg_screen_search_index_remove(self, *args):
            return self.rc

        def pg_screen_search_index_release(self, *args):
            self.released = True
            return 0

        def pg_screen_search_index_import(self, h, shape, kmer, start, member, first, bins, sizes_out):
            if self.rc == 0 and self.sizes is not None:
                import ctypes
                ctypes.memmove(sizes_out, self.sizes.ctypes.data, self.sizes.nbytes)
            return self.rc

        def pg_last_error(self, h):
            return b"stub"
    e = Engine.__new__(Engine)
    e.lib, e._h = Lib(), None
    return e


def test_the_engine_records_a_remove_after_success_only():
    from pyani_amd import _lib
    e = _stub_engine()
    e.screen_search_index([0, 1, 2, 3, 4], 16, 16, labels=["a", "b", "c", "b", "e"])
    e._search["sizes"][:] = [10, 11, 12, 13, 14]
    e._search_q = 5
    e.screen_search_index_remove([])
    assert e._search["n"] == 5 and e._search_q == 5      # nothing removed: nothing dropped
    with pytest.raises(ValueError, match="held by 2 columns"):
        e.screen_search_index_remove(["b"])
    with pytest.raises(ValueError, match="no column"):
        e.screen_search_index_remove(["a", "nobody"])
    with pytest.raises(ValueError, match="a position or a label"):
        e.screen_search_index_remove([1.5])
    assert e._search["n"] == 5
    for rc in (_lib.PG_E_ARG, _lib.PG_E_NOMEM):
        e.lib.rc = rc
        with pytest.raises(_lib.PyaniGpuError):
            e.screen_search_index_remove([0])
        assert e._search["n"] == 5 and len(e._search["labels"]) == 5 and e._search_q == 5
    e.lib.rc = 0
    e.screen_search_index_remove(["a", 3])
    assert e._search["n"] == 3 and e._search["labels"] == ["b", "c", "e"] and e._search["sizes"].tolist() == [11, 12, 14] and e._search_q == 0
    assert (e._search["kmer"], e._search["scale"]) == (16, 16)
    e.screen_search_index_remove(["b"])      # one holder of the label now
    assert e._search["labels"] == ["c", "e"]
    e.screen_search_index_remove([1, 0])
    assert e._search is None      # everything removed: no index
    with pytest.raises(ValueError, match="no search index"):
        e.screen_search_index_remove(["c"])
    with pytest.raises(ValueError, match="no search index"):
        e.screen_search_index_save("nowhere")


def test_the_engine_records_a_load_after_success_only(tmp_path):
    from pyani_amd import _lib, screen
    shape, arrays, sizes, labels, lengths = _file_args(stc.built_index())
    path = tmp_path / "i.idx"
    screen.write_search_index(path, shape, arrays, sizes, labels, lengths)
    e = _stub_engine()
    e.screen_search_index([0, 1], 12, 4, labels=["x", "y"])
    e._search_q = 3
    for rc in (_lib.PG_E_ARG, _lib.PG_E_NOMEM):
        e.lib.rc = rc
        with pytest.raises(_lib.PyaniGpuError):
            e.screen_search_index_load(path)
        assert e._search["labels"] == ["x", "y"] and e._search["kmer"] == 12 and e._search_q == 3
    e.lib.rc, e.lib.sizes = 0, sizes
    got = e.screen_search_index_load(path)
    assert np.array_equal(got[0], sizes) and got[1] == labels and np.array_equal(got[2], lengths) and got[2].dtype == np.uint64
    assert e._search["n"] == shape[0] and (e._search["kmer"], e._search["scale"]) == (shape[1], shape[2]) and e._search["labels"] == labels
    assert np.array_equal(e._search["sizes"], sizes) and e._search_q == 0
    # stored sizes that are not the computed ones: a ValueError, and the index is released
    e.lib.sizes, e.lib.released = sizes + np.uint32(1), False
    with pytest.raises(ValueError, match="stored sizes"):
        e.screen_search_index_load(path)
    assert e.lib.released and e._search is None
    with pytest.raises(ValueError, match="wrong magic"):
        path.write_bytes(b"x" * 200)
        e.screen_search_index_load(path)


def test_the_multi_engine_refuses():
    from pyani_amd.multi import MultiEngine
    m = MultiEngine.__new__(MultiEngine)
    for call in (lambda: m.screen_search_index_save("p"), lambda: m.screen_search_index_load("p"), lambda: m.screen_search_index_remove([0])):
        with pytest.raises(ValueError, match="single Engine"):
            call()


# ---- the drivers' refusals -------------------------------------------------------------------------------------------------------------------
class NoEngine:      # any use would raise AttributeError, not ValueError
    pass


def test_index_refusals_come_before_any_engine(tmp_path, monkeypatch):
    from pyani_amd import screen, subcmd_gather, subcmd_search, subcmd_searchdb

    def no_engine(*a, **kw):
        raise AssertionError("an engine was asked for")
    for mod in (subcmd_search, subcmd_gather, subcmd_searchdb):
        monkeypatch.setattr(mod, "default_engine", no_engine)
    missing = tmp_path / "does_not_exist"
    shape, arrays, sizes, labels, lengths = _file_args(stc.built_index())
    saved = tmp_path / "db.idx"
    screen.write_search_index(saved, shape, arrays, sizes, ["g0", "g1", "g2", "g3"][:shape[0]], lengths)
    drivers = ((subcmd_search.run_screen_search, {"min_identity": 0.8}), (subcmd_gather.run_screen_gather, {"min_unique": 5}))
    for run, args in drivers:
        with pytest.raises(ValueError, match="takes the place of db_dir"):
            run(missing, missing, index=missing, **args)
        with pytest.raises(ValueError, match="a collection is needed"):
            run(None, missing, **args)
        with pytest.raises(ValueError, match="exact="):
            run(None, missing, index=missing, exact="anim", **args)
        with pytest.raises(ValueError, match="db_batch="):
            run(None, missing, index=missing, db_batch=2, **args)
        with pytest.raises(ValueError, match="single Engine"):
            run(None, missing, index=missing, engine=NoEngine(), **args)
    for more in ({"devices": [0, 1]}, {"workers": 2}):
        with pytest.raises(ValueError, match="single Engine"):
            subcmd_search.run_screen_search(None, missing, min_identity=0.8, index=missing, **more)
    # the database drivers
    with pytest.raises(ValueError, match="single Engine"):
        subcmd_searchdb.run_screen_index_build(missing, missing, engine=NoEngine())
    with pytest.raises(ValueError, match="db_batch must be"):
        subcmd_searchdb.run_screen_index_build(missing, missing, db_batch=0)
    with pytest.raises(ValueError, match="k-mer size"):
        subcmd_searchdb.run_screen_index_build(missing, missing, kmer=7)
    with pytest.raises(ValueError, match="single Engine"):
        subcmd_searchdb.run_screen_index_update(saved, engine=NoEngine())
    with pytest.raises(ValueError, match="holds no genome 'nobody'"):
        subcmd_searchdb.run_screen_index_update(saved, remove=["g1", "nobody"])
    with pytest.raises(ValueError, match="given twice"):
        subcmd_searchdb.run_screen_index_update(saved, remove=["g1", "g1"])
    add = tmp_path / "add"
    add.mkdir()
    (add / "g2.fna").write_text(">r\nACGT\n")
    with pytest.raises(ValueError, match="already holds a genome 'g2'"):
        subcmd_searchdb.run_screen_index_update(saved, add_dir=add)


def test_another_kmer_or_scale_than_the_files_is_refused_before_the_import(tmp_path):
    """After the header is read and before anything is uploaded: an Engine without a device whose import would raise AttributeError."""
    from pyani_amd import screen, subcmd_gather, subcmd_search
    from pyani_amd.engine import Engine

    class Idle(Engine):
        def __init__(self):      # no library, no device
            pass

        def genome_count(self):
            return 0

        def clear_genomes(self):
            pass

        def screen_search_index_release(self):
            pass

        def __del__(self):
            pass
    shape, arrays, sizes, labels, lengths = _file_args(stc.built_index())
    saved = tmp_path / "db.idx"
    screen.write_search_index(saved, shape, arrays, sizes, labels, lengths)
    queries = tmp_path / "q"
    queries.mkdir()
    for run, args in ((subcmd_search.run_screen_search, {"min_identity": 0.8}), (subcmd_gather.run_screen_gather, {"min_unique": 5})):
        for other in ({"kmer": shape[1] - 1, "scale": shape[2]}, {"kmer": shape[1], "scale": shape[2] * 2}):
            with pytest.raises(ValueError, match="was built with kmer"):
                run(None, queries, index=saved, engine=Idle(), **other, **args)
