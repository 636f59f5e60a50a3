"""GPU: the profile of a partition over the resident search index — Engine.screen_search_profile against the numpy
statement pyani_amd.screen.profile_of_index and the brute force of tests/screen_profile_cases.py.  Everything is an integer and must be
EQUAL under every tier setting, every batch of the sorted tier and every cut of the index into slices."""
import ctypes

import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_profile_cases as spc

pytestmark = pytest.mark.gpu

NOTHING = {"n": 0, "clusters": 0, "kmers": 0, "entries": 0, "cells": 0, "lane_kmers": 0, "wave_kmers": 0, "sorted_kmers": 0, "sorted_batches": 0, "markers": 0,
           "relabel_ms": 0.0, "lane_ms": 0.0, "wave_ms": 0.0, "sorted_ms": 0.0, "marker_ms": 0.0}


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e
        e.screen_search_profile_set()


def _result(p):
    """A ScreenProfile in the statement's layout."""
    return p.genome_arrays(), p.cluster_arrays(), p.spectrum, p.off, p.marker_arrays()


def _statement(index, label, marker_min_size=2, thresholds=None):
    from pyani_amd import screen
    shape, (kmer, start, member, _, _) = index
    need = thresholds or screen.profile_thresholds(np.bincount(label, minlength=shape[0]))
    return screen.profile_of_index(kmer, start, member, shape[0], label, *need, marker_min_size)


def _under_every_setting(eng, index, label, want, what, marker_min_size=2, thresholds=None, batch_keys=0):
    """The profile under every tier setting equal to `want`; returns the statistics of the last (default) setting."""
    shape = index[0]
    for lane, wave in spc.TIER_SETTINGS:
        eng.screen_search_profile_set(lane, wave, batch_keys)
        p = eng.screen_search_profile(label, marker_min_size=marker_min_size, thresholds=thresholds)
        assert spc.same(_result(p), want) is None, (what, lane, wave, spc.same(_result(p), want))
        last = eng.screen_search_profile_last()
        assert (last["n"], last["kmers"], last["entries"], last["cells"], last["markers"]) == (shape[0], shape[3], shape[4], int(want[1][1].sum()), len(want[4][0])), (what, last)
        assert last["clusters"] == int((label == np.arange(len(label))).sum()) and last["lane_kmers"] + last["wave_kmers"] + last["sorted_kmers"] == shape[3], (what, last)
        if (lane, wave) == (0, 0):
            assert last["sorted_kmers"] == shape[3] and last["lane_ms"] == 0.0, (what, last)
    eng.screen_search_profile_set()
    return last


# ---- every small case: slices, empties, n = 1, the tier edges, the marker logic ---------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(spc.all_cases())), ids=[c[0] for c in spc.all_cases()])
def test_equals_the_statement_and_the_brute_force(eng, case):
    from pyani_amd import screen
    name, index, label = spc.all_cases()[case]
    shape, arrays = index
    sizes = eng.screen_search_index_import(shape, arrays)
    want = _statement(index, label)
    need = screen.profile_thresholds(np.bincount(label, minlength=shape[0]))
    assert spc.same(want, spc.brute(index, label, *need, 2)) is None, name
    last = _under_every_setting(eng, index, label, want, name)
    p = eng.screen_search_profile(label)
    assert (p.held == sizes).all() and p.kmer == shape[1] and p.marker_min_size == 2
    if name.startswith("tiers"):      # the default: h <= 8 a thread, 9, 63 and 64 a wave, 65, 129 and 3000 sorted
        assert (last["wave_kmers"], last["sorted_kmers"], last["sorted_batches"]) == (9, 9, 1), last
        assert last["lane_ms"] > 0.0 and last["wave_ms"] > 0.0 and last["sorted_ms"] > 0.0 and last["marker_ms"] > 0.0 and last["relabel_ms"] > 0.0, last
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


def test_empty_genome(eng):
    index, label = [(i, l) for n, i, l in spc.small_cases() if n == "built_index empty genome"][0]
    eng.screen_search_index_import(*index)
    p = eng.screen_search_profile(label)
    assert all(int(a[3]) == 0 for a in p.genome_arrays()) and int(p.size[3]) == 1 and all(int(a[3]) == 0 for a in p.cluster_arrays()[1:])
    assert p.spectrum_of(3).tolist() == [0]
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


@pytest.mark.parametrize("part", ["mod7", "blocks"])
def test_sorted_batches(eng, part):
    """The sorted tier in batches of at most 1000 entries: the 3000-holder k-mers are batches of their own (larger than the batch), the
    others are cut at k-mer boundaries; under every tier setting."""
    index, label = spc.tiers_index(), spc.tiers_partitions()[part]
    eng.screen_search_index_import(*index)
    want = _statement(index, label)
    last = _under_every_setting(eng, index, label, want, part, batch_keys=1000)
    assert last["sorted_kmers"] == 9 and last["sorted_batches"] >= 4      # the default tiers: 3 x 3000 a batch each, 3 x (65 + 129) in one or more
    eng.screen_search_profile_set(0, 0, 300)
    p = eng.screen_search_profile(label)
    assert spc.same(_result(p), want) is None and eng.screen_search_profile_last()["sorted_batches"] >= 8
    eng.screen_search_profile_set()
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


def test_covered_clusters(eng):
    """The 129-holder k-mer of the genomes 0 ... 128 covers the cluster of 64 and the cluster of 65 exactly: core in both, private in neither."""
    index, label = spc.tiers_index(), spc.tiers_partitions()["blocks"]
    eng.screen_search_index_import(*index)
    p = eng.screen_search_profile(label, marker_min_size=1)
    from tests import screen_store_cases as ssc
    holders = {x: set(hs) for x, hs in ssc.columns_of(index).items()}
    cover = [x for x, hs in holders.items() if hs == set(range(129))]
    assert len(cover) == 1
    for c, members in ((0, set(range(64))), (64, set(range(64, 129)))):
        whole = [x for x, hs in holders.items() if members <= hs]       # the cluster's core cells: every member holds the k-mer
        inside = [x for x, hs in holders.items() if hs <= members]      # its private cells: no holder outside
        assert cover[0] in whole and cover[0] not in inside             # the covering k-mer: core here, private nowhere
        assert (int(p.size[c]), int(p.core[c]), int(p.private[c])) == (len(members), len(whole), len(inside))
        assert int(p.marker[c]) == sum(1 for x in inside if len(holders[x]) >= int(p.core_need[c]))
        assert int(p.spectrum_of(c)[-1]) == len(whole)
        # without the covering k-mer the cluster would have one core cell fewer and as many private ones: the cell is counted exactly so
        assert len([x for x in whole if x != cover[0]]) == int(p.core[c]) - 1
    assert cover[0] not in p.marker_kmer.tolist()
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


def test_marker_logic(eng):
    from pyani_amd import screen
    index, label = spc.marker_index(), spc.marker_label()
    eng.screen_search_index_import(*index)
    position = {x: i for i, x in enumerate(index[1][0].tolist())}
    counted = None
    for min_size, listed in ((1, [3, 2, 2, 1, 2]), (2, [3, 2, 2, 1, 0]), (21, [0, 0, 0, 0, 0])):
        want = _statement(index, label, min_size)
        _under_every_setting(eng, index, label, want, ("marker", min_size), marker_min_size=min_size)
        p = eng.screen_search_profile(label, marker_min_size=min_size)
        assert int(p.core_need[0]) == 19 and np.bincount(p.marker_cluster, minlength=64)[[0, 20, 40, 60, 63]].tolist() == listed
        keys = list(zip(p.marker_cluster.tolist(), [position[x] for x in p.marker_kmer.tolist()]))
        assert keys == sorted(keys)      # the contract's order: ascending cluster, then index position
        assert counted is None or (p.marker == counted).all()      # marker[c] whatever marker_min_size is
        counted = p.marker.copy()
        assert p.marker[[0, 20, 40, 60, 63]].tolist() == [3, 2, 2, 1, 2]
    assert sorted(p.markers_frame().columns) == ["cluster", "kmer", "name", "occupancy"]
    p = eng.screen_search_profile(label, marker_min_size=1)
    assert all(len(t) == 12 and set(t) <= set("ACGT") for t in p.markers_frame()["kmer"]) and len(p.markers_frame()) == 10
    # the directed cells of cluster A: all of A; all of A and an outsider; A without one member; one member and three other clusters
    assert (int(p.core[0]), int(p.private[0]), int(p.marker[0])) == (3, 3, 3) and int(p.foreign[5]) == 1 and int(p.alone[5]) == 1
    c, s = screen.profile_thresholds(np.bincount(label, minlength=64))
    c = c.copy(); c[0] = 20
    want = _statement(index, label, 2, thresholds=(c, s))
    _under_every_setting(eng, index, label, want, "core_need 20", thresholds=(c, s))
    assert int(want[1][6][0]) == 2      # all members but one is no marker where core_need is the size
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


# ---- the scale of the relabel: n = 2^20 ----------------------------------------------------------------------------------------------------------------
def _batches(holders, batch_keys):
    """The batches of the sorted tier over k-mers of `holders` entries in index order: as many k-mers as fit in batch_keys entries, one at least."""
    count, room = 0, 0
    for h in holders:
        if h > room:
            count, room = count + 1, max(batch_keys, h)
        room -= h
    return count


@pytest.mark.parametrize("part", ["pairs", "one"])
def test_million_genomes(eng, part):
    index = spc.million_index()
    n = index[0][0]
    label = (np.arange(n, dtype=np.int32) & ~np.int32(1)) if part == "pairs" else np.zeros(n, dtype=np.int32)
    eng.screen_search_index_import(*index)
    want = _statement(index, label)
    for lane, wave, batch in ((None, None, 0), (0, 0, 1 << 19), (8, 64, 3000)):      # one batch; the k-mer of all a batch of its own; a batch per k-mer
        eng.screen_search_profile_set(lane, wave, batch)
        p = eng.screen_search_profile(label)
        assert spc.same(_result(p), want) is None, (part, lane, wave, batch, spc.same(_result(p), want))
        last = eng.screen_search_profile_last()
        assert (last["clusters"], last["sorted_kmers"]) == (n // 2 if part == "pairs" else 1, 1025), last
        assert last["sorted_batches"] == (_batches(np.diff(index[1][1].astype(np.int64)).tolist(), batch) if batch else 1), last
    eng.screen_search_profile_set()
    eng.screen_search_profile_release()
    eng.screen_search_index_release()


# ---- through the real scan ----------------------------------------------------------------------------------------------------------------------------
REAL = (("family", 16, 16, 0.9), ("edges", 12, 1, 0.9))


@pytest.fixture(scope="module")
def real_engines():
    from pyani_amd.engine import Engine
    out, open_ = {}, []
    for case, _, _, _ in REAL:
        e = Engine(0).__enter__()
        open_.append(e)
        out[case] = (e, [e.add_genome(s, o) for s, o in scr.CASES[case]()])
    yield out
    for e in open_:
        e.__exit__(None, None, None)


def _holders(case, k, scale, which):
    out = {}
    for column, g in enumerate(which):
        seq, off = scr.CASES[case]()[g]
        own = spc.genome_kmers(seq, off, k, scale)
        assert len(own) == len(scr.genome_set(seq, off, k, scale))
        for x in own.tolist():
            out.setdefault(int(x), []).append(column)
    return out


@pytest.mark.parametrize("case,k,scale,identity", REAL)
def test_real_scan(real_engines, case, k, scale, identity):
    from pyani_amd import screen
    e, ids = real_engines[case]
    n = len(ids)
    rep = e.screen_dereplicate(ids, screen.ScreenOptions(identity, k, scale, 2)).rep
    assert len(set(rep.tolist())) < n      # some genomes belong together
    e.screen_search_index(ids, kmer=k, scale=scale)
    _, (kmer, start, member, _, _) = e.screen_search_index_export()
    holders = _holders(case, k, scale, range(n))
    assert set(kmer.tolist()) == set(holders)
    need = screen.profile_thresholds(np.bincount(rep, minlength=n))
    for min_size in (1, 2):
        want = spc.brute_of(kmer.tolist(), holders, n, rep, *need, min_size)
        for lane, wave in spc.TIER_SETTINGS:
            e.screen_search_profile_set(lane, wave, 0)
            p = e.screen_search_profile(rep, marker_min_size=min_size)
            assert spc.same(_result(p), want) is None, (case, min_size, lane, wave, spc.same(_result(p), want))
        e.screen_search_profile_set()
    fresh = _result(e.screen_search_profile(rep))
    assert spc.same(fresh, screen.profile_of_index(kmer, start, member, n, rep, *need, 2)) is None
    # an add: the first genomes indexed, the others added; a remove: all indexed, two removed — each equal to the fresh build over its list
    e.screen_search_index(ids[:n - 2], kmer=k, scale=scale)
    e.screen_search_index_add(ids[n - 2:])
    assert spc.same(_result(e.screen_search_profile(rep)), fresh) is None
    gone = [1, n - 1]
    left = [g for g in range(n) if g not in gone]
    e.screen_search_index_remove(gone)
    first = {}
    sub = np.array([first.setdefault(int(rep[v]), i) for i, v in enumerate(left)], dtype=np.int32)      # the old clusters among the genomes left, named by their first member
    shrunk = _result(e.screen_search_profile(sub))
    e.screen_search_index([ids[g] for g in left], kmer=k, scale=scale)
    assert spc.same(_result(e.screen_search_profile(sub)), shrunk) is None
    sub_need = screen.profile_thresholds(np.bincount(sub, minlength=len(left)))
    _, (kmer2, _, _, _, _) = e.screen_search_index_export()
    assert spc.same(shrunk, spc.brute_of(kmer2.tolist(), _holders(case, k, scale, left), len(left), sub, *sub_need, 2)) is None
    e.screen_search_profile_release()
    e.screen_search_index_release()


# ---- nothing else moves ----------------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(real_engines):
    from pyani_amd import screen
    e, ids = real_engines["family"]
    k, scale = 16, 16
    e.screen_search_profile_release()
    e.screen_search_profile_release()      # nothing resident: still fine
    assert e.screen_search_profile_last() == NOTHING
    e.screen_search_index(ids[:6], kmer=k, scale=scale)
    e.screen_gather_count(ids[6:])
    need_q = np.full(2, 3, dtype=np.uint32)
    sel_before = e.screen_search_select(need_q, np.full(6, 3, dtype=np.uint32))
    rows_before = e.screen_gather_rows(need_q)
    rect_before, left_before, last_before, gather_before = e.screen_search_fetch(), e.screen_gather_fetch(), e.screen_search_last(), e.screen_gather_last()

    def resident(read, like):      # what a read call copies out now, without running anything again
        out = [np.zeros_like(x) for x in like]
        e._check(read(e._h, *(x.ctypes.data if x.size else None for x in out)))
        return out
    exported = e.screen_search_index_export()
    label = np.array([0, 0, 0, 3, 3, 5], dtype=np.int32)
    p = e.screen_search_profile(label, marker_min_size=1)
    assert int(p.held.sum()) == exported[0][4] and e.screen_search_profile_last()["n"] == 6
    assert (e.screen_search_fetch() == rect_before).all() and (e.screen_gather_fetch() == left_before).all()
    assert e.screen_search_last() == last_before and e.screen_gather_last() == gather_before
    assert len(rows_before[0]) > 0 and len(sel_before[0]) > 0
    assert all((x == y).all() for x, y in zip(resident(e.lib.pg_screen_gather_read, rows_before), rows_before))
    assert all((x == y).all() for x, y in zip(resident(e.lib.pg_screen_search_read, sel_before), sel_before))
    again = e.screen_search_index_export()
    assert again[0] == exported[0] and all((x == y).all() for x, y in zip(again[1], exported[1]))
    # the profile reads nothing of the genome store: it survives clear_genomes, as the index does; its engine's genomes are loaded again for the other tests
    want = _result(p)
    e.clear_genomes()
    genomes, clusters, spectrum, markers = e._screen_search_profile_read(6, len(p.marker_kmer))
    assert spc.same((genomes, clusters, spectrum, p.off, markers), want) is None
    assert spc.same(_result(e.screen_search_profile(label, marker_min_size=1)), want) is None      # and so does the index
    ids[:] = [e.add_genome(s, o) for s, o in scr.family()]
    e.screen_search_profile_release()
    e.screen_search_profile_release()
    assert e.screen_search_profile_last() == NOTHING
    e.screen_search_index_release()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from pyani_amd import _lib, screen
    index, label = spc.marker_index(), spc.marker_label()
    n = index[0][0]
    c, s = screen.profile_thresholds(np.bincount(label, minlength=n))
    m = ctypes.c_uint64(7)

    def call(lab=label, core=c, shell=s, nodes=n, min_size=2):
        arrays = [None if x is None else np.ascontiguousarray(x) for x in (lab, core, shell)]      # (alive during the call)
        return eng.lib.pg_screen_search_profile(eng._h, *(None if a is None else a.ctypes.data for a in arrays), nodes, min_size, ctypes.byref(m))

    def refused(text, **kwargs):
        with pytest.raises(_lib.PyaniGpuError, match=text) as err:
            eng._check(call(**kwargs))
        assert err.value.code == _lib.PG_E_ARG

    eng.screen_search_index_release()
    refused("no resident search index")
    with pytest.raises(ValueError, match="no search index on this engine"):
        eng.screen_search_profile(label)
    for fn in (lambda: eng.lib.pg_screen_search_profile_read(eng._h, None, None, None, None, None), lambda: eng.lib.pg_screen_search_profile_read_clusters(eng._h, *[None] * 7),
               lambda: eng.lib.pg_screen_search_profile_read_spectrum(eng._h, None), lambda: eng.lib.pg_screen_search_profile_read_markers(eng._h, None, None, None)):
        with pytest.raises(_lib.PyaniGpuError, match="no resident profile"):
            eng._check(fn())
    eng.screen_search_index_import(*index)
    good = _result(eng.screen_search_profile(label))

    def still_there():
        genomes, clusters, spectrum, markers = eng._screen_search_profile_read(n, len(good[4][0]))
        assert spc.same((genomes, clusters, spectrum, good[3], markers), good) is None

    refused("is of 64 genomes, not 63", nodes=n - 1)
    refused("needs a label", lab=None)
    refused("needs both thresholds", core=None)
    refused("needs both thresholds", shell=None)
    refused("1 member or more, not 0", min_size=0)
    bad = label.copy(); bad[9] = -1
    refused(r"node 9 has the label -1 outside \[0, 64\)", lab=bad)
    bad = label.copy(); bad[9] = n
    refused(r"node 9 has the label 64 outside \[0, 64\)", lab=bad)
    bad = label.copy(); bad[[33, 34]] = 21
    refused("node 33 has the label 21, which does not name itself", lab=bad)
    for which, value in ((0, 21), (1, 0), (1, 20)):      # core_need > size, shell_need < 1, shell_need > core_need
        need = [c.copy(), s.copy()]
        need[which][20] = value
        refused("node 20 names a cluster of 20 with the thresholds", core=need[0], shell=need[1])
        with pytest.raises(ValueError, match="node 20 names a cluster of 20"):
            eng.screen_search_profile(label, thresholds=need)
        still_there()
    assert m.value == 7      # a refusal writes nothing
    for lane, wave in ((9, 64), (4, 65)):
        with pytest.raises(_lib.PyaniGpuError, match="limit is 0 ..."):
            eng.screen_search_profile_set(lane, wave)
    for bad_call in (lambda: eng.screen_search_profile(label[:-1]), lambda: eng.screen_search_profile(label, marker_min_size=0),
                     lambda: eng.screen_search_profile(label, core=0.1, shell=0.2)):
        with pytest.raises(ValueError):
            bad_call()
    still_there()
    # thresholds are read at naming nodes only; any out-pointer may be NULL
    need = [c.copy(), s.copy()]
    need[0][21], need[1][21] = 99, 0
    eng._check(call(core=need[0], shell=need[1]))
    assert m.value == len(good[4][0])
    still_there()
    eng._check(eng.lib.pg_screen_search_profile(eng._h, label.ctypes.data, c.ctypes.data, s.ctypes.data, n, 2, None))
    eng._check(eng.lib.pg_screen_search_profile_read(eng._h, None, None, None, None, None))
    eng._check(eng.lib.pg_screen_search_profile_read_markers(eng._h, None, None, None))
    still_there()
    eng.screen_search_index_release()
    still_there()      # the profile is a state of its own
    eng.screen_search_profile_release()
    assert eng.screen_search_profile_last() == NOTHING


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------------
def test_run_screen_profile(tmp_path):
    import pandas as pd
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_dereplicate import run_dereplicate
    from pyani_amd.subcmd_profile import TABLES, run_screen_profile
    from pyani_amd.subcmd_searchdb import run_screen_index_build
    k, scale = 16, 16
    fam = scr.family()
    db = tmp_path / "db"
    db.mkdir()
    for g in range(6):
        synth.write_fasta(db / f"fam{g}.fna", *fam[g], f"fam{g}")
    with Engine(0) as eng:
        from pyani_amd import screen
        derep = run_dereplicate(db, tmp_path / "derep", screen=screen.ScreenOptions(0.9, k, scale, 2), write_output=True, engine=eng)
        table = [p for p in derep.written if p.name == "screen_clusters.tab"][0]
        a = run_screen_profile(db_dir=db, partition=table, outdir=tmp_path / "from_dir", kmer=k, scale=scale, engine=eng)
        assert [p.name for p in a.written] == [f"profile_{t}.tab" for t in TABLES] and eng.genome_count() == 0 and eng._search is None
        assert eng.screen_search_profile_last()["n"] == 0
        p = a.profile
        stems = [f"fam{g}" for g in range(6)]
        assert p.labels == stems and p.kmer == k and len(a.cluster_names) == len(p.naming())
        rep = derep.clusters.rep
        assert [int(p.label[v]) == int(p.label[w]) for v in range(6) for w in range(6)] == [int(rep[v]) == int(rep[w]) for v in range(6) for w in range(6)]
        assert all(int(p.label[v]) <= v for v in range(6))      # a cluster's naming node is its first member in column order
        frames = (p.genome_frame(), p.cluster_frame(), p.spectrum_frame(), p.markers_frame())
        for path, frame in zip(a.written, frames):
            back = pd.read_csv(path, sep="\t")
            pd.testing.assert_frame_equal(back, frame, check_dtype=False, check_exact=True)
        assert len(frames[3]) > 0 and all(len(t) == k for t in frames[3]["kmer"])
        index = tmp_path / "family.idx"
        run_screen_index_build(db, index, kmer=k, scale=scale, engine=eng)
        named = {s: f"species {int(p.label[v])}" for v, s in enumerate(stems)}
        b = run_screen_profile(index=index, partition=named, outdir=tmp_path / "from_index", engine=eng)
        c = run_screen_profile(db_dir=db, partition=named, outdir=tmp_path / "batched", kmer=k, scale=scale, db_batch=4, engine=eng)
        classes = tmp_path / "classes.txt"
        classes.write_text("".join(f"hash{v}\t{s}\t{named[s]}\n" for v, s in enumerate(stems)))
        d = run_screen_profile(db_dir=db, classes=classes, outdir=tmp_path / "classes", kmer=k, scale=scale, engine=eng)
        assert [x.read_bytes() for x in a.written] == [x.read_bytes() for x in b.written] == [x.read_bytes() for x in c.written] == [x.read_bytes() for x in d.written]
        assert b.cluster_names == sorted(set(named.values()), key=lambda s: int(s.split()[1])) and eng.genome_count() == 0 and eng._search is None
        quiet = run_screen_profile(db_dir=db, partition=named, kmer=k, scale=scale, write_output=False, engine=eng)
        assert quiet.written == [] and spc.same(_result(quiet.profile), _result(p)) is None
        with pytest.raises(ValueError, match="holds no genome 'fam9'"):
            run_screen_profile(db_dir=db, partition={**named, "fam9": "x"}, outdir=tmp_path / "no", engine=eng)
        with pytest.raises(ValueError, match="'fam5' has no class"):
            run_screen_profile(index=index, partition={s: named[s] for s in stems[:5]}, outdir=tmp_path / "no", engine=eng)
        assert not (tmp_path / "no").exists()
