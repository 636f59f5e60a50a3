"""The screen's definition (pyani_amd/csrc/pg_screen_core.h) in numpy, and the inputs of its tests (tests/test_screen_cpu.py,
tests/test_screen_gpu.py).  The k-mers come from tests/sketch_k_cases.record_kmers and the hash from sketch_oracle.mix32, both imported
and unchanged; what is stated here is what the screen adds: ONE set of distinct sampled canonical k-mers per genome, and the matrix of
shared k-mers as the product of the genome x k-mer incidence over the k-mers that two or more genomes hold.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.  Every genome comes from numpy.random.default_rng(seed); every
statement is computed once per (case, k, scale) and shared by the tests of one process."""
import functools

import numpy as np

from tests import sketch_cases as sc      # (puts oracle/ on sys.path)
from tests import sketch_k_cases as skc
from sketch_oracle import mix32           # noqa: E402

N_BINS = 4096
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgtNn", b"TGCAtgcaNn"):
    _COMP[_a] = _b


def revcomp(seq):
    return _COMP[np.asarray(seq, dtype=np.uint8)][::-1].copy()


def genome_occurrences(seq, rec_off, k, scale):
    """Every sampled canonical k-mer OCCURRENCE of a genome (all records, windows of k unambiguous bases inside one record)."""
    out = []
    for r in range(len(rec_off) - 1):
        _, km = skc.record_kmers(np.asarray(seq[int(rec_off[r]):int(rec_off[r + 1])]), k)
        out.append(km[(mix32(km) & np.uint64(scale - 1)) == 0])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def genome_set(seq, rec_off, k, scale):
    """S(g): the distinct sampled canonical k-mers, sorted."""
    return np.unique(genome_occurrences(seq, rec_off, k, scale))


def bin_of(kmers, scale):
    return (mix32(kmers) >> np.uint64(int(scale).bit_length() - 1)) & np.uint64(N_BINS - 1)


def statement(genomes, k, scale):
    """(sizes uint32[n], shared uint32[n, n]) of the definition for [(seq, rec_off)]."""
    sets = [genome_set(s, o, k, scale) for s, o in genomes]
    n = len(sets)
    sizes = np.array([len(x) for x in sets], dtype=np.uint32)
    shared = np.zeros((n, n), dtype=np.int64)
    if n:
        allk = np.concatenate(sets)
        owner = np.concatenate([np.full(len(x), g, dtype=np.int64) for g, x in enumerate(sets)])
        uniq, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
        multi = cnt >= 2                                   # only a k-mer held by two or more genomes adds to an off-diagonal cell
        col = np.cumsum(multi) - 1
        keep = multi[inv]
        inc = np.zeros((n, int(multi.sum())), dtype=np.float64)      # (counts below 2^53: exact)
        inc[owner[keep], col[inv[keep]]] = 1.0
        shared = np.rint(inc @ inc.T).astype(np.int64)
        shared[np.arange(n), np.arange(n)] = sizes
    return sizes, shared.astype(np.uint32)


def identity_of(sizes, shared, k, min_shared=2):
    """The host arithmetic of pyani_amd/screen.py restated: (shared / size[a]) ** (1 / k) where shared >= min_shared, else 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = shared.astype(np.float64) / sizes.astype(np.float64)[:, None]
    ok = shared >= min_shared
    return np.where(ok, np.power(np.where(ok, c, 1.0), 1.0 / k), 0.0)


# ---- family ----------------------------------------------------------------------------------------------------------------------------
FAMILY_PARAMS = ((16, 16), (12, 16), (8, 1), (16, 256))      # (k, scale)
FAMILY_BASES = 60_000
FAMILY_RATES = {1: 0.0, 2: 0.0, 3: 0.02, 4: 0.05, 5: 0.10, 6: 0.03}      # genome -> substitution rate against the ancestor (2: reverse-complemented)
FAMILY_FWD, FAMILY_RC, FAMILY_UNRELATED, FAMILY_DIRTY = 1, 2, 7, 6


@functools.lru_cache(maxsize=None)
def family():
    """0: the ancestor, 3 records with odd boundaries, a 300-base stretch repeated inside its first record (k-mers that occur twice in one
    genome); 1: an exact copy in one record; 2: its reverse complement in one record; 3, 4, 5: copies with 2 %, 5 %, 10 % substitutions in
    2, 3, 1 records; 6: a 3 % copy with an N run and a lower-case stretch; 7: unrelated."""
    rng = np.random.default_rng(20261901)
    n = FAMILY_BASES
    a = sc.random_bases(rng, n)
    a[9_000:9_300] = a[2_000:2_300]
    one = np.array([0, n], dtype=np.uint64)
    dirty = sc.substituted(rng, a, 0.03)
    dirty[30_011:30_050] = ord("N")
    dirty[41_003:43_001] = np.frombuffer(bytes(dirty[41_003:43_001]).lower(), dtype=np.uint8)
    return [(a, sc.offsets(n, 3, 23)), (a.copy(), one), (revcomp(a), one), (sc.substituted(rng, a, 0.02), sc.offsets(n, 2, 7)),
            (sc.substituted(rng, a, 0.05), sc.offsets(n, 3, 11)), (sc.substituted(rng, a, 0.10), one), (dirty, sc.offsets(n, 2, 13)),
            (sc.random_bases(rng, n), sc.offsets(n, 3, 5))]


# ---- wide ------------------------------------------------------------------------------------------------------------------------------
WIDE_N, WIDE_BASES, WIDE_PARAMS = 3000, 48, (16, 1)


@functools.lru_cache(maxsize=None)
def wide():
    """3000 genomes of 48 bases (n is no power of two).  Motif 1 (24 bases: 9 16-mers) is in ALL of them: 9 groups of 3000 genomes,
    9 x 4 498 500 pair increments.  Motif 2 (24 bases) is in genomes 0 and 2999 only: the corner cells.  Motif 3 (20 bases: 5 16-mers)
    stands forward in the genomes with g % 4 == 0 and reverse-complemented in the odd ones.  The rest is random."""
    rng = np.random.default_rng(20261902)
    m1, m2, m3 = sc.random_bases(rng, 24), sc.random_bases(rng, 24), sc.random_bases(rng, 20)
    genomes = []
    off = np.array([0, WIDE_BASES], dtype=np.uint64)
    for g in range(WIDE_N):
        if g == 0:
            rest = m2
        elif g == WIDE_N - 1:
            rest = m2
        elif g % 4 == 0:
            rest = np.concatenate([m3, sc.random_bases(rng, 4)])
        elif g % 2 == 1:
            rest = np.concatenate([sc.random_bases(rng, 4), revcomp(m3)])
        else:
            rest = sc.random_bases(rng, 24)
        genomes.append((np.concatenate([m1, rest] if g % 2 == 0 else [rest, m1]), off))
    return genomes


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
EDGES_PARAMS = (16, 4)
EDGES_SHORT, EDGES_N_ONLY, EDGES_TWIN = 2, 3, 4      # a genome shorter than k; one of N only; genome 0 again


@functools.lru_cache(maxsize=None)
def edges():
    """0: an ancestor of 5 003 bases in 2 records, 1: a 3 % copy, 2: ten bases, 3: 100 N, 4: genome 0 again, 5: unrelated."""
    rng = np.random.default_rng(20261903)
    a = sc.random_bases(rng, 5_003)
    off = sc.offsets(5_003, 2, 3)
    return [(a, off), (sc.substituted(rng, a, 0.03), off), (sc.random_bases(rng, 10), np.array([0, 10], dtype=np.uint64)),
            (np.full(100, ord("N"), dtype=np.uint8), np.array([0, 100], dtype=np.uint64)), (a.copy(), off),
            (sc.random_bases(rng, 4_001), np.array([0, 4_001], dtype=np.uint64))]


# ---- estimate --------------------------------------------------------------------------------------------------------------------------
ESTIMATE_PARAMS = (16, 16)
ESTIMATE_BASES, ESTIMATE_RATES = 200_000, (0.01, 0.03, 0.05, 0.08, 0.10)
ESTIMATE_BOUND = 0.006      # |identity[ancestor][copy] - fraction of unchanged bases|: ~8 sigma of a containment over ~12 400 sampled k-mers


@functools.lru_cache(maxsize=None)
def estimate():
    """Four ancestors of 200 kb, each followed by its substituted copies at ESTIMATE_RATES -> (genomes, [(ancestor, copy, fraction of
    unchanged bases)])."""
    rng = np.random.default_rng(20261904)
    genomes, pairs = [], []
    off = np.array([0, ESTIMATE_BASES], dtype=np.uint64)
    for _ in range(4):
        a = sc.random_bases(rng, ESTIMATE_BASES)
        ia = len(genomes)
        genomes.append((a, off))
        for rate in ESTIMATE_RATES:
            c = sc.substituted(rng, a, rate)
            pairs.append((ia, len(genomes), float((c == a).mean())))
            genomes.append((c, off))
    return genomes, pairs


CASES = {"family": family, "wide": wide, "edges": edges, "estimate": lambda: estimate()[0]}


@functools.lru_cache(maxsize=None)
def expected(case, k, scale):
    """The statement's (sizes, shared) of a case, once per parameter set; the arrays are shared: do not write to them."""
    sizes, shared = statement(CASES[case](), k, scale)
    sizes.setflags(write=False); shared.setflags(write=False)
    return sizes, shared
