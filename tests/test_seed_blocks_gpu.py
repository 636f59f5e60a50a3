"""The two ANIm seeding kernels give the same matches (pga_seed.inc).

anim_seed_kernel probes blocks of up to 32 reference slots per LDS table and streams each query once per block;
anim_seed_pair_kernel (PYANI_SEED_PER_PAIR=1, the fragment mode's kernel) probes one reference per table and streams each
query once per pair.  Hits are appended with atomics in both, so only the per-unit multiset of matches is defined; everything
downstream is a function of it.  Each case compares every alignment record of every pair (pg_anim_alignments_batch) and the
pairs' result tuples between the two kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _both(eng, monkeypatch, pairs, maxmatch=False, block_slots=None):
    """(records, tuples) of the block kernel and of the per-pair kernel for the same call."""
    r = [a for a, _ in pairs]
    q = [b for _, b in pairs]
    out = []
    for per_pair in (False, True):
        if per_pair:
            monkeypatch.setenv("PYANI_SEED_PER_PAIR", "1")
        else:
            monkeypatch.delenv("PYANI_SEED_PER_PAIR", raising=False)
        if block_slots:
            monkeypatch.setenv("PYANI_SEED_BLOCK_SLOTS", str(block_slots))
        off, recs, _, _ = eng.anim_alignments_batch(r, q, maxmatch=maxmatch)
        res = eng.anim_pairs(r, q, maxmatch=maxmatch)
        out.append((off, recs, res))
    monkeypatch.delenv("PYANI_SEED_PER_PAIR", raising=False)
    monkeypatch.delenv("PYANI_SEED_BLOCK_SLOTS", raising=False)
    return out


def _assert_same(got, want, what):
    (o1, r1, t1), (o2, r2, t2) = got, want
    assert np.array_equal(o1, o2), f"{what}: alignment counts per pair differ"
    assert r1.tobytes() == r2.tobytes(), f"{what}: alignment records differ"
    assert t1.tobytes() == t2.tobytes(), f"{what}: pair results differ"


def _prefix(seq, off, n):
    """The first n bases of a genome, records cut accordingly."""
    keep = [int(x) for x in off if int(x) < n]
    return seq[:n].copy(), np.array(keep + [n], dtype=np.uint64)


def test_c4_tile_slice(eng, monkeypatch):
    """Rows x all genomes of the benchmark's set (5 Mb, a few related pairs among unrelated ones): 22 references, i.e. more
    than one block; and again with 2048-slot blocks (blocks of two or three references)."""
    from pyani_amd import synth
    S = synth.SETS["C4"]
    eng.clear_genomes()
    ids = [eng.add_genome(*synth.genome(S["seed"], S["n"], g, S["L"])) for g in range(32)]
    eng.upload()
    pairs = [(a, b) for a in ids[:22] for b in ids]
    new, old = _both(eng, monkeypatch, pairs)
    assert (old[2]["n_alignments"] > 0).sum() >= 22
    _assert_same(new, old, "C4 slice")
    new, old = _both(eng, monkeypatch, pairs[:320], block_slots=2048)
    _assert_same(new, old, "C4 slice, 2048-slot blocks")


def test_family_call_all_pairs_related(eng, monkeypatch):
    """A 25-genome family (one ancestor): every ordered pair related, so both directions of every pair are in the launch and
    one of them is seeded (mirror)."""
    from pyani_amd import synth
    eng.clear_genomes()
    ids = [eng.add_genome(*synth.genome(20250611, 25, g, 1_500_000)) for g in range(25)]
    eng.upload()
    pairs = [(a, b) for a in ids for b in ids if a != b]
    new, old = _both(eng, monkeypatch, pairs)
    assert (old[2]["n_alignments"] > 0).mean() > 0.9
    _assert_same(new, old, "family")


def test_mixed_lengths(eng, monkeypatch):
    """Related genomes of 1 - 12 Mb: blocks of different sizes, references longer than the queries and the reverse."""
    from pyani_amd import synth
    eng.clear_genomes()
    ids = []
    for g, n in enumerate((1_000_000, 3_000_000, 6_000_000, 9_000_000, 12_000_000, 2_000_000)):
        seq, off = synth.genome(20250612, 6, g, 12_000_000)
        ids.append(eng.add_genome(*_prefix(seq, off, min(n, len(seq)))))
    eng.upload()
    pairs = [(a, b) for a in ids for b in ids]
    for mm in (False, True):
        new, old = _both(eng, monkeypatch, pairs, maxmatch=mm)
        assert (old[2]["n_alignments"] > 0).mean() > 0.9
        _assert_same(new, old, f"mixed lengths, maxmatch={mm}")


def test_repetitive_reference_alone_in_its_block(eng, monkeypatch):
    """A genome whose second half is 1 200 tandem copies of a 1 kb unit: its largest groups hold thousands of entries, so with
    2048-slot blocks it is a block of its own (K = 1) and its table is larger than the others'; default blocks too."""
    from pyani_amd import synth
    eng.clear_genomes()
    fam = [synth.genome(20250613, 4, g, 1_000_000) for g in range(4)]
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(5).randint(0, 4, size=1000)]
    seq0, off0 = fam[0]
    flank, foff = _prefix(seq0, off0, 300_000)
    rep = np.concatenate([flank, np.tile(unit, 1200)])
    foff = foff.copy()
    foff[-1] = len(rep)
    ids = [eng.add_genome(rep, foff)] + [eng.add_genome(*fam[g]) for g in range(1, 4)]
    eng.upload()
    pairs = [(a, b) for a in ids for b in ids if a != b] + [(ids[1], ids[1])]
    for slots in (2048, None):
        new, old = _both(eng, monkeypatch, pairs, block_slots=slots)
        assert (old[2]["n_alignments"][:3] > 0).any()
        _assert_same(new, old, f"repetitive reference, block slots {slots}")


def test_small_multi_record_genomes(eng, monkeypatch):
    """Genomes of 20 - 120 kb in many records: most of a query's group slices are empty, so the packed rows of a chunk come from
    a few scattered slices (and a genome too short to seed, one of N only)."""
    from pyani_amd import synth
    eng.clear_genomes()
    ids = []
    for g, n in enumerate((20_000, 45_000, 120_000, 80_000, 60_000, 33_000)):
        seq, _ = synth.genome(20250615, 6, g, 120_000)
        seq = seq[:n].copy()
        ids.append(eng.add_genome(seq, np.arange(0, n + 1, max(1, n // 7), dtype=np.uint64)[:-1].tolist() + [n]))
    ids.append(eng.add_genome(np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8), np.array([0, 14], dtype=np.uint64)))
    ids.append(eng.add_genome(np.frombuffer(b"N" * 5000, dtype=np.uint8), np.array([0, 5000], dtype=np.uint64)))
    eng.upload()
    pairs = [(a, b) for a in ids for b in ids]
    for mm in (False, True):
        new, old = _both(eng, monkeypatch, pairs, maxmatch=mm)
        assert (old[2]["n_alignments"] > 0).sum() >= 12
        _assert_same(new, old, f"small genomes, maxmatch={mm}")


def test_self_pairs_and_pairs_listed_twice(eng, monkeypatch):
    """Self pairs, a pair listed twice and three times (a reference takes further slots for them), both directions, with the
    mirror on and off."""
    from pyani_amd import synth
    eng.clear_genomes()
    ids = [eng.add_genome(*synth.genome(20250614, 5, g, 800_000)) for g in range(5)]
    eng.upload()
    a, b, c, d, e = ids
    odd = [(a, b), (a, b), (b, a), (a, a), (c, d), (d, c), (a, b), (b, b), (c, e), (e, c), (c, e), (d, a), (a, d)]
    for no_mirror in (False, True):
        if no_mirror:
            monkeypatch.setenv("PYANI_ANIM_NO_MIRROR", "1")
        for mm in (False, True):
            new, old = _both(eng, monkeypatch, odd, maxmatch=mm)
            assert (old[2]["n_alignments"] > 0).mean() > 0.9
            _assert_same(new, old, f"odd pairs, no_mirror={no_mirror}, maxmatch={mm}")
        monkeypatch.delenv("PYANI_ANIM_NO_MIRROR", raising=False)
