"""The sketch mode's definition with the k-mer size as a parameter (pyani_amd/csrc/pg_sketch_core.h, 8 <= k <= 16), in numpy, and the
inputs of the general-k tests (tests/test_sketch_k_cpu.py, tests/test_sketch_k_gpu.py).  It follows oracle/sketch_oracle.py line for
line with K replaced by k (tests/test_sketch_k_cpu.py ties the two together at k = 16), and adds the root of the general case.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.  Every genome comes from numpy.random.default_rng(seed); every
sketch is built once per (case, genome, k, frag_len, scale) and shared by the tests of one process."""
import functools
import math

import numpy as np

from tests import sketch_cases as sc      # (puts oracle/ on sys.path)
from sketch_oracle import _CODE, mix32    # noqa: E402

MIN_IDENTITY = 0.80
NEWTON_STEPS = 12
K_MIN, K_MAX = 8, 16


def record_words(seq_bytes, k):
    """(start positions, forward words, reverse-complement words) of every window of k unambiguous bases of one record."""
    codes = _CODE[np.asarray(seq_bytes, dtype=np.uint8)]
    n = len(codes)
    if n < k:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    ok = codes < 4
    c = np.where(ok, codes, 0).astype(np.uint64)
    fwd = np.zeros(n - k + 1, dtype=np.uint64)
    rc = np.zeros(n - k + 1, dtype=np.uint64)
    bad = np.zeros(n - k + 1, dtype=np.int64)
    for i in range(k):      # first base in the HIGH bits of the 2k-bit field; rc: the complement of the LAST base in the high bits
        fwd |= c[i:n - k + 1 + i] << np.uint64(2 * (k - 1 - i))
        rc |= (np.uint64(3) - c[k - 1 - i:n - i]) << np.uint64(2 * (k - 1 - i))
        bad += (~ok[i:n - k + 1 + i]).astype(np.int64)
    pos = np.nonzero(bad == 0)[0]
    return pos, fwd[pos], rc[pos]


def record_kmers(seq_bytes, k):
    """(start positions, canonical k-mers) of every window of k unambiguous bases of one record (numpy uint8 of ASCII)."""
    pos, fwd, rc = record_words(seq_bytes, k)
    return pos, np.minimum(fwd, rc)


def genome_sketch(seq, rec_off, k, frag_len=3000, scale=16):
    """seq: uint8 ASCII of the records back to back, rec_off: record boundaries.
    -> (set of sampled canonical k-mers, per-fragment arrays of sampled k-mer occurrences, number of fragments, k)"""
    kset, frags = set(), []
    for r in range(len(rec_off) - 1):
        rec = np.asarray(seq[int(rec_off[r]):int(rec_off[r + 1])])
        pos, km = record_kmers(rec, k)
        keep = (mix32(km) & np.uint64(scale - 1)) == 0
        pos, km = pos[keep], km[keep]
        kset.update(int(x) for x in km)
        n_full = len(rec) // frag_len
        j = pos // frag_len
        inside = (j < n_full) & ((pos - j * frag_len + k) <= frag_len)
        for f in range(n_full):
            frags.append(km[inside & (j == f)])
    return kset, frags, len(frags), k


def frag_identity(h, n, k):
    """(h / n)^(1/k) as the definition computes it, in float64 (scalars or arrays): k = 16 four square roots; k = 8 ... 15 those four
    roots as the start, then exactly NEWTON_STEPS steps p = y; k - 2 times p = p * y; y = y - (p * y - c) / (k * p)."""
    c = np.asarray(h, dtype=np.float64) / np.asarray(n, dtype=np.float64)
    y = np.sqrt(np.sqrt(np.sqrt(np.sqrt(c))))
    if k != 16:
        kd = np.float64(k)
        for _ in range(NEWTON_STEPS):
            p = y
            for _ in range(k - 2):
                p = p * y
            y = y - (p * y - c) / (kd * p)
    return y if y.ndim else float(y)


def sketch_pair(query_sketch, ref_sketch, k, min_fraction=0.2):
    """(ani fraction, matches, fragments, status) of one ordered pair: the definition, in its order (fragments ascending)."""
    _, frags, nf, kq = query_sketch
    assert kq == k and ref_sketch[3] == k
    rset = ref_sketch[0]
    total, matches = 0.0, 0
    for occ in frags:
        n = len(occ)
        if n == 0:
            continue
        h = sum(1 for x in occ if int(x) in rset)
        if h < 2:
            continue
        ident = math.sqrt(math.sqrt(math.sqrt(math.sqrt(h / n)))) if k == 16 else frag_identity(h, n, k)
        if ident >= MIN_IDENTITY:
            total = total + ident
            matches += 1
    enough = matches > 0 and float(matches) >= min_fraction * float(nf)
    return (total / matches if enough else 0.0, matches, nf, 0 if enough else 1)


# ---- the root's grid (tests 2 and 3) ---------------------------------------------------------------------------------------------------
def identity_grid():
    """(h, n) int64 arrays: every 2 <= h <= n <= 400, then h in {2, n / 2, n} at n in {1000, 2985, 4096} — in that order."""
    hs, ns = [], []
    for n in range(2, 401):
        hs.append(np.arange(2, n + 1)); ns.append(np.full(n - 1, n))
    for n in (1000, 2985, 4096):
        hs.append(np.array([2, n // 2, n])); ns.append(np.full(3, n))
    return np.concatenate(hs).astype(np.int64), np.concatenate(ns).astype(np.int64)


# ---- parameter sets and genomes of the GPU cases (non-vacuity is checked on the definition alone by the CPU tests) --------------------------
#            k, bases, frag_len, scale, min_fraction
K_PARAMS = ((8, 3_000, 64, 4, 0.5), (11, 60_000, 256, 16, 0.5), (12, 120_000, 1000, 16, 0.2), (15, 120_000, 3000, 16, 0.2))


@functools.lru_cache(maxsize=None)
def family(k):
    """0: an ancestor in 3 records with odd boundaries, 1: a copy with 3 % substitutions, 2: unrelated; all 9 ordered pairs."""
    _, size, _, _, _ = next(p for p in K_PARAMS if p[0] == k)
    rng = np.random.default_rng(20261000 + k)
    off = sc.offsets(size, 3, 23)
    a = sc.random_bases(rng, size)
    genomes = [(a, off), (sc.substituted(rng, a), off), (sc.random_bases(rng, size), off)]
    return sc.Case(f"family_k{k}", genomes, [(q, r) for q in range(3) for r in range(3)], {(q, r) for q in (0, 1) for r in (0, 1)} | {(2, 2)})


@functools.lru_cache(maxsize=None)
def more_queries():
    """Three more genomes beside family(12) for the several-devices call: a 3 % copy of the ancestor's first 50 kb, two unrelated."""
    rng = np.random.default_rng(20261099)
    a = family(12).genomes[0][0]
    return [(sc.substituted(rng, a[:50_000]), sc.offsets(50_000, 2, 7)), (sc.random_bases(rng, 40_013), sc.offsets(40_013, 2, 5)),
            (sc.random_bases(rng, 30_000), np.array([0, 30_000], dtype=np.uint64))]


def record_lengths(k):
    """sketch_cases.RECORD_LENGTHS taken around THIS k."""
    return (0, 1, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def records(k):
    """sketch_cases.records() with the record lengths around k (frag_len 64): empty records first, last and twice in a row; N runs across
    the first and the second fragment boundary; one record in lower case.  1: the same sequence as ONE plain record."""
    rng = np.random.default_rng(20261200 + k)
    lengths = [0]
    for rep in range(24):
        lengths += list(record_lengths(k))
        lengths += [int(x) for x in rng.integers(130, 700, size=3)]
    lengths += [0, 0, 257, 0]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    plain = sc.random_bases(rng, int(off[-1]))
    seq = plain.copy()
    long_recs = [r for r, n in enumerate(lengths) if n >= 200]
    for r in long_recs[::5]:
        seq[int(off[r]) + 60:int(off[r]) + 70] = ord("N")
        seq[int(off[r]) + 125:int(off[r]) + 160] = ord("N")
    r = long_recs[2]
    seq[int(off[r]):int(off[r + 1])] = np.frombuffer(bytes(seq[int(off[r]):int(off[r + 1])]).lower(), dtype=np.uint8)
    genomes = [(seq, off), (plain, np.array([0, len(plain)], dtype=np.uint64))]
    case = sc.Case(f"records_k{k}", genomes, [(0, 0), (0, 1), (1, 0), (1, 1)], {(0, 0), (0, 1), (1, 0), (1, 1)})
    case.lengths = lengths
    return case


@functools.lru_cache(maxsize=None)
def case_fn(kind, k):
    """The zero-argument callable of a case (what k_sketch / k_pair / sketch_cases.non_vacuity's callers are keyed by)."""
    return functools.partial({"family": family, "records": records}[kind], k)


# ---- the definition's answers, computed once -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k_sketch(case_fn, g, k, frag_len, scale):
    case = case_fn()
    seq, off = case.genomes[g]
    # (a genome that is only ever a reference is sketched without fragments, as sketch_cases.oracle_sketch does)
    return genome_sketch(seq, off, k, frag_len=frag_len if g in case.queries else 1 << 40, scale=scale)


@functools.lru_cache(maxsize=None)
def k_pair(case_fn, q, r, k, frag_len, scale, min_fraction):
    return sketch_pair(k_sketch(case_fn, q, k, frag_len, scale), k_sketch(case_fn, r, k, frag_len, scale), k, min_fraction)


def k_pairs(case_fn, k, frag_len, scale, min_fraction, pairs=None):
    return [k_pair(case_fn, q, r, k, frag_len, scale, float(min_fraction)) for q, r in (case_fn().pairs if pairs is None else pairs)]
