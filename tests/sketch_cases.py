"""Inputs and expected values of the sketch-mode shape tests (tests/test_sketch_shapes_cpu.py, tests/test_sketch_shapes_gpu.py): genomes
that take pg_sketch_pairs (pyani_amd/csrc/pg_sketch.hip) off its default path, and the numpy definition's answer for them
(oracle/sketch_oracle.py, unchanged).  A plain helper module: every genome comes from numpy.random.default_rng(seed), every oracle sketch
is built once per (case, genome, frag_len, scale) and shared by the tests of one process.  Test infrastructure only."""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "oracle") not in sys.path:
    sys.path.insert(0, str(ROOT / "oracle"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# ---- the launch shape pg_sketch_pairs chooses, restated from its host code ("jobs: the pairs by query, up to SK_REFS references per
# workgroup"): per_ref = max(n_frags, 1) * 4 bytes; more than 96 KiB: PG_E_CAPACITY; g_max = min(SK_REFS, 96 KiB / per_ref) references
# per job; dynamic LDS of a job = per_ref * (its references); above 48 KiB the kernel's limit is raised (hipFuncSetAttribute) --------------
SK_REFS = 4
LDS_DEFAULT = 48 * 1024
LDS_LIMIT = 96 * 1024
MAX_QUERY_FRAGMENTS = LDS_LIMIT // 4      # 24 576


def n_fragments(rec_off, frag_len):
    return int(sum((int(b) - int(a)) // frag_len for a, b in zip(rec_off[:-1], rec_off[1:])))


def per_ref_bytes(n_frags):
    return max(n_frags, 1) * 4


def refs_per_job(n_frags):
    """g_max of pg_sketch_pairs; 0: the query is refused (PG_E_CAPACITY)."""
    return 0 if per_ref_bytes(n_frags) > LDS_LIMIT else min(SK_REFS, LDS_LIMIT // per_ref_bytes(n_frags))


def job_sizes(n_frags, n_refs):
    """How pg_sketch_pairs cuts one query's n_refs references into jobs, e.g. 7 references at g_max 3: [3, 3, 1]."""
    g = refs_per_job(n_frags)
    return [min(g, n_refs - a) for a in range(0, n_refs, g)]


def lds_bytes(n_frags, n_refs):
    """Dynamic LDS of the largest job of one query with n_refs references."""
    return per_ref_bytes(n_frags) * max(job_sizes(n_frags, n_refs))


# ---- genomes -------------------------------------------------------------------------------------------------------------------------
def random_bases(rng, n):
    return ACGT[rng.integers(0, 4, size=n)]


def substituted(rng, seq, rate=0.03):
    """A copy with `rate` of the positions replaced by a DIFFERENT base."""
    out = seq.copy()
    at = np.nonzero(rng.random(len(seq)) < rate)[0]
    code = np.searchsorted(ACGT, out[at])
    out[at] = ACGT[(code + rng.integers(1, 4, size=len(at))) % 4]
    return out


def offsets(total, n_rec, odd):
    """n_rec record boundaries over `total` bases; the inner boundaries are moved by odd amounts: no record length is a multiple of 32."""
    cut = [0] + [total * r // n_rec + odd * r for r in range(1, n_rec)] + [total]
    return np.array(cut, dtype=np.uint64)


class Case:
    """genomes: [(seq, rec_off)]; pairs: [(query index, reference index)] in call order; related: the pairs whose genomes share an ancestor."""

    def __init__(self, name, genomes, pairs, related=()):
        self.name, self.genomes, self.pairs, self.related = name, genomes, list(pairs), set(related)
        self.queries = sorted({q for q, _ in self.pairs})

    def fragments(self, k, frag_len):
        return n_fragments(self.genomes[k][1], frag_len)


# sizes of the mixed call at frag_len 64: (bases, records, odd shift) -> fragments ~ bases / 64
MIXED_SIZES = {"small": (120_000, 2, 7), "lds96_4refs": (300_000, 3, 11), "3refs": (450_000, 3, 13), "2refs": (600_000, 2, 17), "1ref": (900_000, 3, 19)}
MIXED_EXPECT = {"small": (4, False), "lds96_4refs": (4, True), "3refs": (3, True), "2refs": (2, True), "1ref": (1, True)}   # (g_max, more than 48 KiB)


@functools.lru_cache(maxsize=None)
def mixed():
    """Five ancestors (one per size class of pg_sketch_pairs' job cutting at frag_len 64), a 3 % copy of each, one unrelated genome.  Every
    ancestor is a query against itself, its copy, the unrelated genome and the four other families' copies: 7 references each, so the
    3-per-job query is cut 3 + 3 + 1 and the 2-per-job query 2 + 2 + 2 + 1.  The pair list is shuffled and holds one pair twice."""
    rng = np.random.default_rng(20260101)
    genomes, anc, cop = [], {}, {}
    for name, (size, n_rec, odd) in MIXED_SIZES.items():
        off = offsets(size, n_rec, odd)
        a = random_bases(rng, size)
        anc[name] = len(genomes); genomes.append((a, off))
        cop[name] = len(genomes); genomes.append((substituted(rng, a), off))
    unrelated = len(genomes); genomes.append((random_bases(rng, 100_037), offsets(100_037, 2, 5)))
    pairs, related = [], set()
    for name in MIXED_SIZES:
        q = anc[name]
        refs = [q, cop[name], unrelated] + [cop[o] for o in MIXED_SIZES if o != name]
        pairs += [(q, r) for r in refs]
        related |= {(q, q), (q, cop[name])}
    order = np.random.default_rng(7).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    pairs.append(pairs[3])      # one pair twice in a call
    case = Case("mixed", genomes, pairs, related)
    case.ancestor = anc
    return case


LIMIT_BASES = MAX_QUERY_FRAGMENTS * 64      # 1 572 864


@functools.lru_cache(maxsize=None)
def limit():
    """0: one record of exactly 24 576 fragments of 64 (the largest accepted query); 1: the same with 64 bases more (24 577: refused as a
    query, fine as a reference); 2: a small 3 % relative of the first 100 kb (a query that is always valid)."""
    rng = np.random.default_rng(20260102)
    big = random_bases(rng, LIMIT_BASES + 64)
    small = substituted(rng, big[:100_000])
    genomes = [(big[:LIMIT_BASES].copy(), np.array([0, LIMIT_BASES], dtype=np.uint64)), (big, np.array([0, LIMIT_BASES + 64], dtype=np.uint64)),
               (small, offsets(100_000, 2, 9))]
    return Case("limit", genomes, [(0, 0), (0, 1), (2, 1), (2, 0), (0, 2), (2, 2)], {(0, 0), (0, 1), (2, 1), (2, 0), (0, 2), (2, 2)})


PROD_BASES, PROD_FRAG_LEN, PROD_SCALE = 17_500_000, 3000, 64
SCAN_CHUNK_POSITIONS = 8 * 256 * 32      # build_sketch: the scan grid is at most num_cu * 8 workgroups of 256 lanes, 32 start positions per lane


@functools.lru_cache(maxsize=None)
def production():
    """0: 17.5 Mb in two records (its stream is longer than one pass of the scan kernel's grid on 256 compute units: a second grid-stride
    trip; ~5 800 fragments of 3 000: more than 48 KiB of LDS); 1: a 3 % copy of one 2 Mb window of it; 2: unrelated."""
    rng = np.random.default_rng(20260103)
    big = random_bases(rng, PROD_BASES)
    genomes = [(big, np.array([0, 8_700_011, PROD_BASES], dtype=np.uint64)), (substituted(rng, big[9_000_000:11_000_000]), np.array([0, 2_000_000], dtype=np.uint64)),
               (random_bases(rng, 200_003), np.array([0, 200_003], dtype=np.uint64))]
    return Case("production", genomes, [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0)], {(0, 0), (0, 1), (1, 0)})


RECORD_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 79, 80, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def records():
    """0: several hundred records at frag_len 64 — the lengths around k = 16 and around one and two fragments, mixed with longer ones, so
    that most 32-position chunks of the scan hold one or more record boundaries; empty records first, last and twice in a row; N runs
    across fragment boundaries; one record in lower case.  1: the same sequence as ONE plain record."""
    rng = np.random.default_rng(20260104)
    lengths = [0]
    for rep in range(24):
        lengths += list(RECORD_LENGTHS)
        lengths += [int(x) for x in rng.integers(130, 700, size=3)]
    lengths += [0, 0, 257, 0]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    plain = random_bases(rng, int(off[-1]))
    seq = plain.copy()
    long_recs = [r for r, n in enumerate(lengths) if n >= 200]
    for r in long_recs[::5]:      # an N run across the record's first, and across its second, fragment boundary
        seq[int(off[r]) + 60:int(off[r]) + 70] = ord("N")
        seq[int(off[r]) + 125:int(off[r]) + 160] = ord("N")
    r = long_recs[2]
    seq[int(off[r]):int(off[r + 1])] = np.frombuffer(bytes(seq[int(off[r]):int(off[r + 1])]).lower(), dtype=np.uint8)
    genomes = [(seq, off), (plain, np.array([0, len(plain)], dtype=np.uint64))]
    case = Case("records", genomes, [(0, 0), (0, 1), (1, 0), (1, 1)], {(0, 0), (0, 1), (1, 0), (1, 1)})
    case.lengths = lengths
    return case


EDGE_PARAMS = ((3000, 1), (3000, 4096), (64, 16), (65, 16))
EQUALITY_PARAMS = (64, 4)      # the min_fraction comparison at equality is made on pair EQUALITY_PAIR at these parameters
EQUALITY_PAIR = (0, 1)


@functools.lru_cache(maxsize=None)
def edges():
    """A 120 kb family: 0 the ancestor (3 records), 1 and 2 copies with 3 % substitutions, 3 unrelated; all ordered pairs."""
    rng = np.random.default_rng(20260105)
    off = offsets(120_000, 3, 23)
    a = random_bases(rng, 120_000)
    genomes = [(a, off), (substituted(rng, a), off), (substituted(rng, a), offsets(120_000, 2, 3)), (random_bases(rng, 120_000), off)]
    fam = (0, 1, 2)
    return Case("edges", genomes, [(q, r) for q in range(4) for r in range(4)], {(q, r) for q in fam for r in fam} | {(3, 3)})


@functools.lru_cache(maxsize=None)
def replacement():
    """A genome unrelated to everything in edges(): what is added under id 0 after clear_genomes()."""
    rng = np.random.default_rng(20260106)
    a = random_bases(rng, 90_011)
    return (a, offsets(90_011, 2, 29)), (substituted(rng, a), offsets(90_011, 2, 29))


# ---- the definition's answers, computed once ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_sketch(case_fn, k, frag_len, scale):
    """sketch_oracle.genome_sketch of genome k of a case, once per parameter set."""
    import sketch_oracle as so
    case = case_fn()
    seq, off = case.genomes[k]
    # a genome's k-mer SET does not depend on frag_len (genome_sketch samples before it cuts): a genome that is only ever a reference
    # is sketched without fragments, which skips the oracle's per-fragment loop and nothing else
    return so.genome_sketch(seq, off, frag_len=frag_len if k in case.queries else 1 << 40, scale=scale)


@functools.lru_cache(maxsize=None)
def oracle_pair(case_fn, q, r, frag_len, scale, min_fraction):
    """(ani, matches, fragments, status) of the definition for genomes q (query) and r (reference) of a case."""
    import sketch_oracle as so
    return so.sketch_pair(oracle_sketch(case_fn, q, frag_len, scale), oracle_sketch(case_fn, r, frag_len, scale), min_fraction)


def oracle_pairs(case_fn, frag_len, scale, min_fraction, pairs=None):
    return [oracle_pair(case_fn, q, r, frag_len, scale, float(min_fraction)) for q, r in (case_fn().pairs if pairs is None else pairs)]


def assert_records_equal(res, want, what):
    """matches, fragments and status equal, the ANI estimate bit-equal (as test_sketch_pairs_equal_the_definition_bit_for_bit does)."""
    assert len(res) == len(want), what
    for k, (r, (ani, matches, frags, status)) in enumerate(zip(res, want)):
        assert (int(r["matches"]), int(r["fragments"]), int(r["status"])) == (matches, frags, status), (what, k, r, (ani, matches, frags, status))
        assert float(r["ani"]).hex() == float(ani).hex(), (what, k, float(r["ani"]), ani)


def non_vacuity(case, want, pairs=None):
    """The conditions under which a comparison with the oracle means something: at least half of the related pairs have a result with half
    of the fragments matching, every unrelated pair has none.  Returns (related with a strong result, related, unrelated)."""
    pairs = case.pairs if pairs is None else pairs
    strong = related = unrelated = 0
    for (q, r), (ani, matches, frags, status) in zip(pairs, want):
        if (q, r) in case.related:
            related += 1
            strong += status == 0 and 2 * matches >= frags and ani > 0.0
        else:
            unrelated += 1
            assert status == 1 and ani == 0.0, (case.name, q, r, matches, frags)
    assert related and 2 * strong >= related, (case.name, strong, related)
    return strong, related, unrelated
