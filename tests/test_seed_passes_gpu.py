"""Seeding in passes (pyani_amd/csrc/pg_seed_plan.h, pga_seed.inc): a reference k-mer group that holds more entries than half the
LDS table is cut into passes, each filled and probed by the same query stream.  Every (reference entry, query entry) hit is found
in exactly one pass, so the per-unit multiset of matches, the only thing downstream depends on (tests/test_seed_blocks_gpu.py),
is that of a table large enough.

  * forced passes (PYANI_SEED_MAX_SLOTS = 256 and 2048, a development knob) give the bytes of the same call without the knob: both
    seeding kernels, --mum and --maxmatch, fragment mode;
  * at production defaults, a genome whose most frequent 16-mer occurs more than 8192 times (a 9000-copy tandem of a 40-base unit)
    is a reference of ANIm and a subject of ANIb like any other: records and tuples equal the independent nucmer oracle's
    (oracle/nucmer_oracle.cpp, oracle/anim_oracle.py) and the CPU statement's (oracle/anib_cpu.py).  Before passes existed every call
    with R in the table role (ANIm reference, ANIb subject) returned PG_E_CAPACITY; the calls with R streamed only are regression
    cases;
  * the plan itself (PYANI_SEED_PLAN_LOG, a development log line per seeding launch): the knob sets the table and forces the passes
    the byte comparisons rely on, out-of-range values are ignored, and R takes passes at production defaults.

Not tested: the refusal of a reference of 2^30 - 1 or more bases (the block table's 30 position bits).  The check sits in the host
planner behind the upload of the genome and its seed lists, so reaching it needs a gigabase genome on the device."""
import functools
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KNOBS = ("PYANI_SEED_MAX_SLOTS", "PYANI_SEED_PER_PAIR", "PYANI_ANIM_NO_MIRROR", "PYANI_SEED_PLAN_LOG")


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _no_knobs_left(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _prefix(seq, off, n):
    """The first n bases of a genome, records cut accordingly."""
    keep = [int(x) for x in off if int(x) < n]
    return seq[:n].copy(), np.array(keep + [min(n, len(seq))], dtype=np.uint64)


def _append(genome, tail):
    """`tail` appended to the genome's last record."""
    seq, off = genome
    off = np.array(off, dtype=np.uint64)
    off[-1] = len(seq) + len(tail)
    return np.concatenate([seq, tail]), off


@functools.lru_cache(maxsize=None)
def _family_a():
    """Four 300 kb relatives; genome 0 is cut to 150 kb and extended by 600 tandem copies of a random 1 kb unit, genome 1 carries the
    same tandem in its middle: a repeat on BOTH sides (every probe of a pass walks a long chain of equal keys)."""
    from pyani_amd import synth
    fam = [synth.genome(20250701, 4, g, 300_000) for g in range(4)]
    tandem = np.tile(ACGT[np.random.RandomState(11).randint(0, 4, size=1000)], 600)
    g0 = _append(_prefix(*fam[0], 150_000), tandem)
    seq1, off1 = fam[1]
    mid = len(seq1) // 2
    g1 = (np.concatenate([seq1[:mid], tandem, seq1[mid:]]),
          np.array([int(x) if int(x) <= mid else int(x) + len(tandem) for x in off1], dtype=np.uint64))
    return [g0, g1, fam[2], fam[3]]


@functools.lru_cache(maxsize=None)
def _small_genomes():
    """The multi-record 20 - 120 kb genomes, the 14-base genome and the all-N genome of test_seed_blocks_gpu.py."""
    from pyani_amd import synth
    out = []
    for g, n in enumerate((20_000, 45_000, 120_000, 80_000, 60_000, 33_000)):
        seq, _ = synth.genome(20250615, 6, g, 120_000)
        out.append((seq[:n].copy(), np.array(np.arange(0, n + 1, max(1, n // 7), dtype=np.uint64)[:-1].tolist() + [n], dtype=np.uint64)))
    out.append((np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8), np.array([0, 14], dtype=np.uint64)))
    out.append((np.frombuffer(b"N" * 5000, dtype=np.uint8), np.array([0, 5000], dtype=np.uint64)))
    return out


@functools.lru_cache(maxsize=None)
def _odd_family():
    from pyani_amd import synth
    return [synth.genome(20250614, 5, g, 800_000) for g in range(5)]


def _load(eng, genomes):
    eng.clear_genomes()
    ids = [eng.add_genome(*g) for g in genomes]
    eng.upload()
    return ids


def _anim(eng, monkeypatch, pairs, maxmatch, per_pair, max_slots):
    """(offsets, alignment records, result tuples) of one ANIm call under the given seeding kernel and largest table."""
    monkeypatch.setenv("PYANI_SEED_PER_PAIR", "1" if per_pair else "0")
    if max_slots:
        monkeypatch.setenv("PYANI_SEED_MAX_SLOTS", str(max_slots))
    else:
        monkeypatch.delenv("PYANI_SEED_MAX_SLOTS", raising=False)
    r, q = [a for a, _ in pairs], [b for _, b in pairs]
    off, recs, _, _ = eng.anim_alignments_batch(r, q, maxmatch=maxmatch)
    res = eng.anim_pairs(r, q, maxmatch=maxmatch)
    monkeypatch.delenv("PYANI_SEED_MAX_SLOTS", raising=False)
    return off, recs, res


def _assert_same(got, want, what):
    (o1, r1, t1), (o2, r2, t2) = got, want
    assert np.array_equal(o1, o2), f"{what}: alignment counts per pair differ"
    assert r1.tobytes() == r2.tobytes(), f"{what}: alignment records differ"
    assert t1.tobytes() == t2.tobytes(), f"{what}: pair results differ"


def _forced_equal_plain(eng, monkeypatch, pairs, maxmatch, per_pair, what):
    plain = _anim(eng, monkeypatch, pairs, maxmatch, per_pair, None)
    for slots in (256, 2048):
        _assert_same(_anim(eng, monkeypatch, pairs, maxmatch, per_pair, slots), plain, f"{what}, {slots} slots")
    return plain


KERNELS = pytest.mark.parametrize("per_pair", [False, True], ids=["block", "per_pair"])
MODES = pytest.mark.parametrize("maxmatch", [False, True], ids=["mum", "maxmatch"])


@KERNELS
@MODES
def test_forced_passes_same_bytes_repeat_on_both_sides(eng, monkeypatch, per_pair, maxmatch):
    """Family (a): at 256 slots the coarse groups of a 300 kb genome (about 146 entries) need two passes and the tandem's fine groups
    (600 equal keys each) five or more; at 2048 slots only the tandem's groups need more than one."""
    ids = _load(eng, _family_a())
    pairs = [(a, b) for a in ids for b in ids if a != b]
    plain = _forced_equal_plain(eng, monkeypatch, pairs, maxmatch, per_pair, "family with a tandem on both sides")
    assert (plain[2]["n_alignments"] > 0).sum() >= 6


@KERNELS
@MODES
def test_forced_passes_same_bytes_small_multi_record_genomes(eng, monkeypatch, per_pair, maxmatch):
    ids = _load(eng, _small_genomes())
    pairs = [(a, b) for a in ids for b in ids]
    plain = _forced_equal_plain(eng, monkeypatch, pairs, maxmatch, per_pair, "small genomes")
    assert (plain[2]["n_alignments"] > 0).sum() >= 12


@KERNELS
@MODES
@pytest.mark.parametrize("no_mirror", [False, True], ids=["mirror", "no_mirror"])
def test_forced_passes_same_bytes_self_pairs_and_pairs_listed_twice(eng, monkeypatch, per_pair, maxmatch, no_mirror):
    a, b, c, d, e = _load(eng, _odd_family())
    odd = [(a, b), (a, b), (b, a), (a, a), (c, d), (d, c), (a, b), (b, b), (c, e), (e, c), (c, e), (d, a), (a, d)]
    if no_mirror:
        monkeypatch.setenv("PYANI_ANIM_NO_MIRROR", "1")
    plain = _forced_equal_plain(eng, monkeypatch, odd, maxmatch, per_pair, f"odd pairs, no_mirror={no_mirror}")
    assert (plain[2]["n_alignments"] > 0).mean() > 0.9


def test_forced_passes_same_bytes_fragment_mode(eng, monkeypatch):
    """ANIb on family (a): pair tuples and batched row tables under the knob equal the same calls without it, byte for byte.
    The two pairs with the tandem on BOTH sides (genomes 0 and 1) are left out: tandem against tandem gives ~1200 maximal matches of
    hundreds of kb that overlap on the query, and the fragment stage after seeding sizes a unit's clipped-seed range as matches +
    fragments (anib_frag_stage), which holds only when a fragment boundary is crossed by few matches; anib_bucket_kernel then
    writes past the range.  That is a bug of the fragment stage, reachable with or without passes and not touched here (DESIGN.md §6
    names it and the fix it needs); the ANIm cases above cover the repeat on both sides."""
    ids = _load(eng, _family_a())
    pairs = [(a, b) for a in ids for b in ids if a != b and {a, b} != {ids[0], ids[1]}]
    q, s = [a for a, _ in pairs], [b for _, b in pairs]

    def run(slots):
        if slots:
            monkeypatch.setenv("PYANI_SEED_MAX_SLOTS", str(slots))
        else:
            monkeypatch.delenv("PYANI_SEED_MAX_SLOTS", raising=False)
        res = eng.anib_pairs(q, s)
        bres, off, rows = eng.anib_rows_batch(q, s)
        monkeypatch.delenv("PYANI_SEED_MAX_SLOTS", raising=False)
        return res, bres, off, rows

    plain = run(None)
    assert (plain[0]["status"] == 0).all() and (plain[0]["n_kept"] > 0).sum() >= 6 and int(plain[2][-1]) > 1000
    for slots in (256, 2048):
        got = run(slots)
        for name, x, y in zip(("pair tuples", "batch tuples", "row offsets", "rows"), got, plain):
            assert x.tobytes() == y.tobytes(), f"fragment mode, {slots} slots: {name} differ"


def _plans(capfd, call):
    """The [seed-plan] lines (PYANI_SEED_PLAN_LOG: kernel, table slots, most passes of a group) of the seeding launches `call` makes."""
    capfd.readouterr()
    call()
    lines = [ln.split() for ln in capfd.readouterr().err.splitlines() if ln.startswith("[seed-plan]")]
    assert lines, "no seeding launch was logged"
    return [(t[1].split("=")[1], int(t[2].split("=")[1]), int(t[3].split("=")[1])) for t in lines]


@KERNELS
def test_the_knob_sets_the_table_and_forces_passes(eng, monkeypatch, capfd, per_pair):
    """What makes the byte comparisons above comparisons of passes: under PYANI_SEED_MAX_SLOTS the planned table has that many slots and
    family (a) needs several passes (256 slots: 128 entries a pass against the tandem's groups of 600 equal keys, five at least; 2048
    slots: two at least, a tandem group with two of the unit's k-mers holds 1200), without it one pass; a value that is no power of
    two from 256 to 16384 is ignored."""
    ids = _load(eng, _family_a())
    r, q = [a for a in ids for b in ids if a != b], [b for a in ids for b in ids if a != b]
    monkeypatch.setenv("PYANI_SEED_PLAN_LOG", "1")
    monkeypatch.setenv("PYANI_SEED_PER_PAIR", "1" if per_pair else "0")
    kernel = "per_pair" if per_pair else "block"
    plain = _plans(capfd, lambda: eng.anim_pairs(r, q))
    assert all(k == kernel and slots > 2048 and passes == 1 for k, slots, passes in plain), plain
    for slots, least in ((256, 5), (2048, 2)):
        monkeypatch.setenv("PYANI_SEED_MAX_SLOTS", str(slots))
        got = _plans(capfd, lambda: eng.anim_pairs(r, q))
        assert all(k == kernel and s == slots and passes >= least for k, s, passes in got), (slots, got)
    for bad in ("128", "300", "32768", "-256", "x"):
        monkeypatch.setenv("PYANI_SEED_MAX_SLOTS", bad)
        assert _plans(capfd, lambda: eng.anim_pairs(r, q)) == plain, bad


def test_the_tandem_genome_takes_passes_at_production_defaults(eng, monkeypatch, capfd):
    """No table knob: with R as ANIm reference (block kernel) and as ANIb subject (per-pair kernel) the plan is the largest table and
    more than one pass; with B as the reference and R as the query it is one pass (R's lists are only streamed)."""
    fam = _tandem_family()
    ids = dict(zip(fam, _load(eng, list(fam.values()))))
    monkeypatch.setenv("PYANI_SEED_PLAN_LOG", "1")
    got = _plans(capfd, lambda: eng.anim_pairs([ids["R"]], [ids["B"]]))
    assert all(k == "block" and slots == 16384 and passes >= 2 for k, slots, passes in got), got
    got = _plans(capfd, lambda: eng.anib_pairs([ids["B"]], [ids["R"]]))
    assert all(k == "per_pair" and slots == 16384 and passes >= 2 for k, slots, passes in got), got
    got = _plans(capfd, lambda: eng.anim_pairs([ids["B"]], [ids["R"]]))
    assert all(k == "block" and passes == 1 for k, slots, passes in got), got


# ---- production defaults: a genome no single table holds --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tandem_family():
    """R: the first 300 kb of a family member followed, in its last record, by 9000 copies of a 40-base unit (660 kb); B, C: two relatives
    without the tandem."""
    from pyani_amd import synth
    fam = [synth.genome(20250702, 4, g, 300_000) for g in range(3)]
    unit = ACGT[np.random.RandomState(5).randint(0, 4, 40)]
    return {"R": _append(_prefix(*fam[0], 300_000), np.tile(unit, 9000)), "B": fam[1], "C": fam[2]}


def _most_frequent_16mer(seq):
    code = np.full(256, 4, dtype=np.uint64)
    code[ACGT] = np.arange(4, dtype=np.uint64)
    c = code[seq]
    n = len(c) - 15
    k = np.zeros(n, dtype=np.uint64)
    dirty = np.zeros(n, dtype=bool)
    for j in range(16):
        k |= (c[j:j + n] & np.uint64(3)) << np.uint64(2 * j)
        dirty |= c[j:j + n] == 4
    return int(np.unique(k[~dirty], return_counts=True)[1].max())


def test_premise_one_16mer_beyond_half_the_largest_table():
    """What makes R a genome the single-pass kernels refuse: one 16-mer alone (let alone its group) outgrows the 8192 entries that a
    16384-slot table takes."""
    assert _most_frequent_16mer(_tandem_family()["R"][0]) > 8192


@pytest.fixture(scope="module")
def tandem_fastas(tmp_path_factory):
    from tests.fuzz_genomes import write_fasta
    d = tmp_path_factory.mktemp("seed_passes")
    out = {}
    for name, (seq, off) in _tandem_family().items():
        out[name] = d / f"{name}.fna"
        write_fasta(out[name], f"{name}_", [seq[int(off[i]):int(off[i + 1])].tobytes().decode() for i in range(len(off) - 1)])
    return out


@pytest.fixture(scope="module")
def nucmer_oracle():
    """(reference, query, maxmatch) -> the oracle's records with record ordinals for names, in its output order; each pair run once."""
    from tests.test_anim_filter_oracle_cpu import oracle_records
    from tests.test_anim_multirecord_gpu import _oracle
    exe = _oracle()
    cache = {}

    def records(fastas, a, b, maxmatch):
        if (a, b, maxmatch) not in cache:
            orc = oracle_records(exe, fastas[a], fastas[b], ["--maxmatch"] if maxmatch else [])
            cache[(a, b, maxmatch)] = [(int(r[0][len(a) + 1:]), int(r[1][len(b) + 1:])) + r[2:] for r in orc]
        return cache[(a, b, maxmatch)]
    return records


def _check_anim_call(eng, fastas, oracle, ids, names, maxmatch):
    """One call on the ordered pairs `names`: every record's coordinates and error count, the kept flags and the filtered tuple equal
    the oracle's records through oracle/anim_oracle.py's delta-filter -1 and parse_delta."""
    from tests.stress_genomes import expected_filtered
    from tests.test_anim_filter_oracle_gpu import _check
    r, q = [ids[a] for a, _ in names], [ids[b] for _, b in names]
    off, recs, _, _ = eng.anim_alignments_batch(r, q, maxmatch=maxmatch)
    res = eng.anim_pairs(r, q, maxmatch=maxmatch)
    n = 0
    for k, (a, b) in enumerate(names):
        want = oracle(fastas, a, b, maxmatch)
        keep, tup = expected_filtered([(str(w[0]), str(w[1])) + tuple(w[2:]) for w in want])
        assert int(res[k]["status"]) == 0 or tup is None, (a, b, res[k])
        _check(f"{a} vs {b}, maxmatch={maxmatch}", k, want, keep, tup, recs[int(off[k]):int(off[k + 1])], res[k])
        n += len(want)
    return n


def test_anim_at_production_defaults_equals_the_nucmer_oracle(eng, monkeypatch, tandem_fastas, nucmer_oracle):
    """R as the reference of B and C in one call, B and C as references against R (R is only streamed there: one pass, a regression
    case), both directions in one call (mirror); --mum, and --maxmatch for (R, B).  No knob is set: the block kernel at its default
    table, R alone in its block and seeded in passes (test_the_tandem_genome_takes_passes_at_production_defaults)."""
    fam = _tandem_family()
    ids = dict(zip(fam, _load(eng, list(fam.values()))))
    n = _check_anim_call(eng, tandem_fastas, nucmer_oracle, ids, [("R", "B"), ("R", "C")], False)
    assert n >= 60      # (the oracle's own count: 300 kb relatives with indels and rearrangements give tens of records a pair)
    _check_anim_call(eng, tandem_fastas, nucmer_oracle, ids, [("B", "R"), ("C", "R")], False)
    _check_anim_call(eng, tandem_fastas, nucmer_oracle, ids, [("R", "B"), ("R", "C"), ("B", "R"), ("C", "R")], False)
    assert _check_anim_call(eng, tandem_fastas, nucmer_oracle, ids, [("R", "B")], True) >= 30


def test_anib_at_production_defaults_equals_the_cpu_statement(eng):
    """B vs R (R is the subject: its coarse groups outgrow the table) and R vs B: tables equal oracle/anib_cpu.py's row for row, tuples
    equal reduce_rows, and pg_anib_rows_batch on the two pairs equals the single-pair tables."""
    import anib_cpu
    from tests.test_anib_gpu import _rows
    fam = _tandem_family()
    ids = dict(zip(fam, _load(eng, list(fam.values()))))
    names = [("B", "R"), ("R", "B")]
    res = eng.anib_pairs([ids[a] for a, _ in names], [ids[b] for _, b in names])
    single = []
    for (a, b), r in zip(names, res):
        want = anib_cpu.anib_cpu_pair(fam[a], fam[b])
        got = eng.anib_pair_rows(ids[a], ids[b])
        assert _rows(got) == _rows(want) and len(want) > 100, (a, b, len(got), len(want))
        aln, err, pid, kept = anib_cpu.reduce_rows(want)
        assert (int(r["aln_length"]), int(r["sim_errors"]), int(r["n_kept"])) == (aln, err, len(kept)), (a, b)
        assert abs(float(r["pid"]) - pid) <= 1e-12 * max(1.0, pid) and int(r["status"]) == 0
        single.append(got)
    bres, off, rows = eng.anib_rows_batch([ids[a] for a, _ in names], [ids[b] for _, b in names])
    assert [tuple(r) for r in bres] == [tuple(r) for r in res]
    for k, got in enumerate(single):
        assert _rows(rows[int(off[k]):int(off[k + 1])]) == _rows(got), names[k]
