"""CPU-only: the profile's statement (pyani_amd.screen.profile_of_index) against an independent brute force in dicts and
sets on every small case, the exact thresholds, the spectrum's identities, the k-mer text and the readers of a partition."""
from fractions import Fraction

import numpy as np
import pytest

from pyani_amd import screen
from tests import screen_cases as scr
from tests import screen_profile_cases as spc
from tests import sketch_k_cases as skc


def _statement(index, label, marker_min_size=2, core=0.95, shell=0.15, thresholds=None):
    shape, (kmer, start, member, _, _) = index
    n = shape[0]
    need = thresholds or screen.profile_thresholds(np.bincount(label, minlength=n), core, shell)
    return screen.profile_of_index(kmer, start, member, n, label, *need, marker_min_size), need


@pytest.mark.parametrize("case", range(len(spc.all_cases())), ids=[c[0] for c in spc.all_cases()])
def test_statement_equals_brute_force(case):
    name, index, label = spc.all_cases()[case]
    for min_size in (1, 2):
        got, need = _statement(index, label, min_size)
        assert spc.same(got, spc.brute(index, label, *need, min_size)) is None, (name, min_size)
    got, need = _statement(index, label, 2, core=1.0, shell=0.5)
    assert spc.same(got, spc.brute(index, label, *need, 2)) is None, name


def test_empty_genome_and_one_genome():
    cases = {c[0]: c for c in spc.small_cases()}
    _, index, label = cases["built_index empty genome"]
    (genomes, clusters, spectrum, off, _), _ = _statement(index, label)
    assert all(int(a[3]) == 0 for a in genomes) and int(clusters[0][3]) == 1 and all(int(a[3]) == 0 for a in clusters[1:])
    assert int(spectrum[off[3]]) == 0
    _, index, label = cases["one genome"]
    (genomes, clusters, spectrum, _, markers), _ = _statement(index, label, 1)
    assert [int(a[0]) for a in genomes] == [7, 7, 7, 7, 0] and [int(a[0]) for a in clusters] == [1, 7, 7, 7, 0, 7, 7] and spectrum.tolist() == [7]
    assert len(markers[0]) == 7 and (markers[1] == index[1][0]).all()
    (_, _, _, _, markers), _ = _statement(index, label, 2)
    assert len(markers[0]) == 0


@pytest.mark.parametrize("size", [1, 2, 19, 20, 21, 100, 1 << 20])
def test_thresholds(size):
    for core, shell in ((0.95, 0.15), (1.0, 1.0), (0.5, 0.5), (0.95, 1e-9), (1.0, 0.15)):
        c, s = screen.profile_thresholds([size, 0, size], core, shell)
        assert c.dtype == s.dtype == np.uint32 and c[1] == s[1] == 0 and c[0] == c[2] and s[0] == s[2]
        for got, fraction in ((int(c[0]), Fraction(core)), (int(s[0]), Fraction(shell))):
            # the smallest integer need >= 1 with need >= fraction * size, in exact rational arithmetic
            assert got >= 1 and Fraction(got) >= fraction * size and (got == 1 or Fraction(got - 1) < fraction * size), (size, core, shell)
        assert 1 <= int(s[0]) <= int(c[0]) <= size
    c, s = screen.profile_thresholds([size])
    want = {1: (1, 1), 2: (2, 1), 19: (19, 3), 20: (19, 3), 21: (20, 4), 100: (95, 15), 1 << 20: (996148, 157287)}[size]      # 0.95 and 0.15 as floats lie a hair below and above
    assert (int(c[0]), int(s[0])) == want


@pytest.mark.parametrize("core, shell", [(0.95, 0.0), (0.95, -0.1), (1.01, 0.15), (0.1, 0.15), (float("nan"), 0.15), (0.95, float("nan")), ("x", 0.15)])
def test_thresholds_refused(core, shell):
    with pytest.raises(ValueError, match="0 < shell <= core <= 1"):
        screen.profile_thresholds([3], core, shell)


def test_statement_refusals():
    index, label = spc.marker_index(), spc.marker_label()
    shape, (kmer, start, member, _, _) = index
    n = shape[0]
    c, s = screen.profile_thresholds(np.bincount(label, minlength=n))
    bad = label.copy(); bad[7] = n
    with pytest.raises(ValueError, match=r"node 7 has the label 64 outside \[0, 64\)"):
        screen.profile_of_index(kmer, start, member, n, bad, c, s)
    bad = label.copy(); bad[30] = 1
    with pytest.raises(ValueError, match="node 30 has the label 1, which does not name itself"):
        screen.profile_of_index(kmer, start, member, n, bad, c, s)
    for which, value in ((0, 21), (1, 0), (1, 20)):      # core_need > size, shell_need < 1, shell_need > core_need
        need = [c.copy(), s.copy()]
        need[which][20] = value
        with pytest.raises(ValueError, match="node 20 names a cluster of 20 with the thresholds"):
            screen.profile_of_index(kmer, start, member, n, label, *need)
    need = [c.copy(), s.copy()]
    need[0][21], need[1][21] = 99, 0      # read at naming nodes only
    assert spc.same(screen.profile_of_index(kmer, start, member, n, label, *need), screen.profile_of_index(kmer, start, member, n, label, c, s)) is None
    for m in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="marker_min_size"):
            screen.profile_of_index(kmer, start, member, n, label, c, s, m)
    with pytest.raises(ValueError, match="not those of a search index"):
        screen.profile_of_index(kmer, start, member, n - 1, label[:-1], c[:-1], s[:-1])


@pytest.mark.parametrize("case", range(len(spc.all_cases())), ids=[c[0] for c in spc.all_cases()])
def test_spectrum_identities(case):
    _, index, label = spc.all_cases()[case]
    (genomes, clusters, spectrum, off, markers), need = _statement(index, label, 1)
    size, kmers, core, soft, shell, private, marker = clusters
    shape, (_, start, member, _, _) = index
    assert int(spectrum.sum()) == int(kmers.sum()) and int(size.sum()) == shape[0]
    for c in np.flatnonzero(size).tolist():
        row = spectrum[off[c]:off[c] + int(size[c])]
        assert int(row.sum()) == int(kmers[c]) and int(row[-1]) == int(core[c])
        assert int(row[int(need[0][c]) - 1:].sum()) == int(soft[c])                                # the upper tail
        assert int(row[int(need[1][c]) - 1:int(need[0][c]) - 1].sum()) == int(shell[c])
    assert (genomes[0] == screen.search_index_sizes(member, shape[0])).all()                       # held = the index's sizes
    assert (genomes[4] <= genomes[3]).all() and (genomes[3] <= genomes[0]).all() and (marker <= private).all() and (marker <= soft).all() and (core <= soft).all()
    assert len(markers[0]) == int(marker.sum())                                                    # marker_min_size 1 lists every marker
    p = screen.profile_from_arrays(None, label, *need, 1, genomes, clusters, spectrum, markers, kmer=shape[1])
    assert (p.off == off).all() and all((p.spectrum_of(c) == spectrum[off[c]:off[c] + int(size[c])]).all() for c in p.naming().tolist())
    g, c, s, m = p.genome_frame(), p.cluster_frame(), p.spectrum_frame(), p.markers_frame()
    assert (g["singleton"] == (genomes[3].astype(np.int64) - genomes[4])).all() and (g["core_missing"] == soft[label].astype(np.int64) - genomes[1]).all()
    assert (np.isnan(g["core_fraction"]) == (soft[label] == 0)).all()
    assert (c["cloud"] == (kmers - soft - shell)[p.naming()].astype(np.int64)).all() and (c["cloud"] >= 0).all()
    assert int(s["kmers"].sum()) == int(kmers.sum()) and (s["kmers"] > 0).all() and len(m) == len(markers[0])


def test_marker_logic_in_the_statement():
    index, label = spc.marker_index(), spc.marker_label()
    position = {x: i for i, x in enumerate(index[1][0].tolist())}
    got = {}
    for min_size in (1, 2, 21):
        (_, clusters, _, _, markers), need = _statement(index, label, min_size)
        assert int(need[0][0]) == 19      # profile_thresholds(core=0.95) at size 20
        got[min_size] = (clusters[6].copy(), markers)
        keys = list(zip(markers[0].tolist(), [position[x] for x in markers[1].tolist()]))
        assert keys == sorted(keys)      # ascending cluster, then index position
    assert all((got[m][0] == got[1][0]).all() for m in (2, 21))      # marker[c] whatever marker_min_size is
    assert got[1][0][[0, 20, 40, 60, 63]].tolist() == [3, 2, 2, 1, 2]
    assert np.bincount(got[1][1][0], minlength=64)[[0, 20, 40, 60, 63]].tolist() == [3, 2, 2, 1, 2]
    assert np.bincount(got[2][1][0], minlength=64)[[0, 20, 40, 60, 63]].tolist() == [3, 2, 2, 1, 0]
    assert len(got[21][1][0]) == 0
    # with core_need 20 the k-mer of all members but one is no marker any more
    c, s = screen.profile_thresholds(np.bincount(label, minlength=64))
    c = c.copy(); c[0] = 20
    (genomes, clusters, _, _, _), _ = _statement(index, label, 2, thresholds=(c, s))
    assert int(clusters[6][0]) == 2 and int(clusters[2][0]) == 3 and int(clusters[5][0]) == 3      # markers, core, private of A
    assert int(genomes[4][5]) == 1 and int(genomes[3][5]) == 1 and int(genomes[4].sum()) >= 4      # the foreign k-mer of genome 5


def test_kmer_string():
    seq, off = scr.edges()[0]
    text = bytes(seq).decode()
    for k, scale in ((16, 4), (12, 1), (8, 1)):
        rec = np.asarray(seq[int(off[0]):int(off[1])])
        pos, fwd, rc = skc.record_words(rec, k)
        canon = np.minimum(fwd, rc)
        for i in (0, 1, len(pos) // 2, len(pos) - 1):
            s = screen.kmer_string(int(canon[i]), k)
            assert len(s) == k and set(s) <= set("ACGT")
            assert s in text or bytes(scr.revcomp(np.frombuffer(s.encode(), dtype=np.uint8))).decode() in text
            assert s == text[int(pos[i]):int(pos[i]) + k] if fwd[i] <= rc[i] else s == bytes(scr.revcomp(rec[int(pos[i]):int(pos[i]) + k])).decode()
            # the canonical form is the smaller code: the text's own code, and the code of its reverse complement, in the tests' encoding
            back = skc.record_words(np.frombuffer(s.encode(), dtype=np.uint8), k)
            assert int(back[1][0]) == int(canon[i]) and int(back[1][0]) <= int(back[2][0])
    assert screen.kmer_string(0, 8) == "AAAAAAAA" and screen.kmer_string(4 ** 16 - 1, 16) == "T" * 16 and screen.kmer_string(0b00011011, 4) == "ACGT"
    for value, k in ((4 ** 8, 8), (-1, 8), (0, 0), (0, 17)):
        with pytest.raises(ValueError):
            screen.kmer_string(value, k)


def test_partition_readers(tmp_path):
    from pyani_amd import subcmd_profile as sp
    table = tmp_path / "clusters.tab"
    table.write_text("genome\trepresentative\tvia\ng0\tg0\t0\ng1\tg0\t17\n# a comment\n\ng2\tg2\t0\n")
    assert sp.read_partition(table) == {"g0": "g0", "g1": "g0", "g2": "g2"} == sp.read_partition({"g0": "g0", "g1": "g0", "g2": "g2"})
    classes = tmp_path / "classes.txt"
    classes.write_text("abc\tg0\tspecies A\ndef\tg1\tspecies B\n012\tg2\tspecies A\n")
    named = sp.read_classes(classes)
    assert named == {"g0": "species A", "g1": "species B", "g2": "species A"}
    label, names = sp.partition_labels(["g2", "g1", "g0"], named)
    assert label.tolist() == [0, 1, 0] and label.dtype == np.int32 and names == ["species A", "species B"]      # the first member in column order names
    table.write_text("g0\tx\ng0\ty\n")
    with pytest.raises(ValueError, match="'g0' is given twice"):
        sp.read_partition(table)
    classes.write_text("abc\tg0\tA\ndef\tg0\tB\n")
    with pytest.raises(ValueError, match="'g0' is given twice"):
        sp.read_classes(classes)
    for text in ("abc\tg0\n", "abc\tg0\t \n"):
        classes.write_text(text)
        with pytest.raises(ValueError, match="'g0' has no class"):
            sp.read_classes(classes)
    table.write_text("g0\n")
    with pytest.raises(ValueError, match="no cluster column"):
        sp.read_partition(table)
    with pytest.raises(ValueError, match="'g1' has no class"):
        sp.read_partition({"g0": "x", "g1": ""})
    with pytest.raises(ValueError, match="holds no genome 'g9'"):
        sp.partition_labels(["g0", "g1"], {"g0": "x", "g1": "x", "g9": "y"})
    with pytest.raises(ValueError, match="'g1' has no class"):
        sp.partition_labels(["g0", "g1"], {"g0": "x"})
    # the driver refuses before any device work (no engine is made: none could be, here)
    for kwargs, text in (({"db_dir": tmp_path}, "partition= or classes="), ({"db_dir": tmp_path, "partition": {}, "classes": classes}, "partition= or classes="),
                         ({"partition": {}}, "db_dir= or index="), ({"db_dir": tmp_path, "index": tmp_path / "x", "partition": {}}, "db_dir= or index="),
                         ({"db_dir": tmp_path, "partition": {}, "write_output": True}, "output directory"),
                         ({"db_dir": tmp_path, "partition": {}, "outdir": tmp_path, "core": 0.1, "shell": 0.2}, "0 < shell <= core <= 1"),
                         ({"db_dir": tmp_path, "partition": {}, "outdir": tmp_path, "marker_min_size": 0}, "marker_min_size"),
                         ({"db_dir": tmp_path, "partition": {"nobody": "x"}, "outdir": tmp_path}, "holds no genome 'nobody'")):
        with pytest.raises(ValueError, match=text):
            sp.run_screen_profile(**kwargs)


def test_multi_engine_refuses():
    from pyani_amd import multi
    with pytest.raises(ValueError, match="single Engine"):
        multi.MultiEngine.screen_search_profile(object(), [0])
    for name in ("screen_search_profile_last", "screen_search_profile_release", "screen_search_profile_set"):
        with pytest.raises(ValueError, match="single Engine"):
            getattr(multi.MultiEngine, name)(object())
