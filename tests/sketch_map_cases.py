"""The MAPPED sketch mode's definition (mapping = "window": pyani_amd/csrc/pg_sketch_core.h, "MAPPED variant") in numpy / plain Python,
and the inputs of its tests (tests/test_sketch_map_cpu.py, tests/test_sketch_map_gpu.py).  Built on tests/sketch_k_cases.py
(record_kmers, genome_sketch, frag_identity) and sketch_oracle.mix32, which are imported and left as they are.  TEST INFRASTRUCTURE
ONLY: nothing under pyani_amd/ imports this file.  Every genome comes from numpy.random.default_rng(seed); every answer is computed once
per process and shared.

The definition, with L = frag_len: a sampled k-mer occurrence of the reference has the coordinate g = its start in the records back to
back WITHOUT separator; bin g // L of nb = ceil(genome length / L); window w (0 <= w < nb) = bins w and w + 1.  Per query fragment: for
every sampled occurrence x (with multiplicity) B(x) = the bins its k-mer occurs in; c_b = occurrences with b in B(x), h_w = occurrences
with B(x) meeting {w, w + 1}; h = max h_w, w* the lowest window reaching it, bin = w* if c_w* >= c_(w* + 1) else w* + 1 (both -1 at
h = 0); identity = frag_identity(h, n, k); candidate iff n > 0, h >= 2, identity >= 0.80; per bin the larger identity wins, ties to
the lowest fragment; ANI = the survivors' identities summed in fragment order / their number."""
import functools

import numpy as np

from tests import sketch_cases as sc
from tests import sketch_k_cases as skc
from sketch_oracle import mix32    # noqa: E402  (tests.sketch_cases put the directory on sys.path)

MIN_IDENTITY = skc.MIN_IDENTITY
MAX_BINS = 8192            # pg_sketch.hip MAP_MAX_BINS: bins per reference at frag_len <= 65 535 (4 096 above)
TOUCH_LIST = 512           # pg_sketch.hip MAP_TOUCH: bins a wave lists per fragment before it scans the whole counter array


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def reference_bins(seq, rec_off, k, frag_len, scale):
    """({canonical sampled k-mer: ascending array of the DISTINCT bins it occurs in}, nb) of a genome in the reference role."""
    total = int(rec_off[-1])
    nb = -(-total // frag_len)
    kms, gs = [], []
    for r in range(len(rec_off) - 1):
        lo, hi = int(rec_off[r]), int(rec_off[r + 1])
        pos, km = skc.record_kmers(np.asarray(seq[lo:hi]), k)
        keep = (mix32(km) & np.uint64(scale - 1)) == 0
        kms.append(km[keep]); gs.append(pos[keep] + lo)      # records back to back: no separator base in the coordinate
    km = np.concatenate(kms) if kms else np.zeros(0, dtype=np.uint64)
    b = (np.concatenate(gs) if gs else np.zeros(0, dtype=np.int64)) // frag_len
    order = np.lexsort((b, km))
    km, b = km[order], b[order]
    out = {}
    if len(km):
        cuts = np.flatnonzero(np.diff(km)) + 1
        for key, bins in zip(km[np.concatenate([[0], cuts])], np.split(b, cuts)):
            out[int(key)] = np.unique(bins)
    return out, nb


def map_fragment(occ, bins, nb):
    """(window, bin, h, window ties, windows touched) of one fragment's occurrence array."""
    c = np.zeros(nb + 2, dtype=np.int64)
    h = np.zeros(nb + 1, dtype=np.int64)
    touched = set()
    for x in occ:
        B = bins.get(int(x))
        if B is None:
            continue
        c[B] += 1
        W = np.union1d(B, B - 1)
        h[W[W >= 0]] += 1
        touched.update(int(v) for v in B)
    hmax = int(h[:nb].max()) if nb else 0
    if hmax == 0:
        return -1, -1, 0, 0, 0
    w = int(np.argmax(h[:nb]))      # the lowest window that reaches the maximum
    ties = int(np.count_nonzero(h[:nb] == hmax))
    return w, (w if c[w] >= c[w + 1] else w + 1), hmax, ties, len(touched)


def mapped_pair(frags, bins, nb, k, min_fraction=0.2):
    """((ani, matches, fragments, status), per-fragment records (window, bin, hits, n, identity, kept), statistics of the rules used)."""
    recs, best = [], {}
    stats = dict(window_tie=0, bin_up=0, dropped=0, identity_tie=0, low_identity=0, few_hits=0, list_overflow=0)
    for f, occ in enumerate(frags):
        n = len(occ)
        w, b, h, ties, touched = map_fragment(occ, bins, nb) if n else (-1, -1, 0, 0, 0)
        ident = float(skc.frag_identity(h, n, k)) if (n > 0 and h >= 2) else 0.0
        stats["window_tie"] += ties > 1
        stats["bin_up"] += h > 0 and b == w + 1
        stats["few_hits"] += h < 2
        stats["low_identity"] += h >= 2 and ident < MIN_IDENTITY
        stats["list_overflow"] += touched > TOUCH_LIST
        recs.append([w, b, h, n, ident, 0])
        if ident >= MIN_IDENTITY:
            if b not in best or ident > best[b][0]:      # ties: the lowest fragment index stays
                best[b] = (ident, f)
    total, matches = 0.0, 0
    for f, r in enumerate(recs):
        if r[4] >= MIN_IDENTITY:
            if best[r[1]][1] == f:
                r[5] = 1
                total = total + r[4]
                matches += 1
            else:
                stats["dropped"] += 1
                stats["identity_tie"] += best[r[1]][0] == r[4]
    nf = len(frags)
    enough = matches > 0 and float(matches) >= min_fraction * float(nf)
    return (total / matches if enough else 0.0, matches, nf, 0 if enough else 1), [tuple(r) for r in recs], stats


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
#                    k: bases, frag_len, scale, min_fraction
FAMILY_PARAMS = {8: (3_000, 64, 4, 0.5), 12: (120_000, 1000, 16, 0.2), 16: (120_000, 3000, 16, 0.2)}


@functools.lru_cache(maxsize=None)
def family(k):
    """sketch_k_cases.family's shape: 0 an ancestor in 3 records with odd boundaries, 1 a 3 % copy, 2 unrelated; all 9 ordered pairs."""
    size = FAMILY_PARAMS[k][0]
    rng = np.random.default_rng(20261300 + k)
    off = sc.offsets(size, 3, 23)
    a = sc.random_bases(rng, size)
    genomes = [(a, off), (sc.substituted(rng, a), off), (sc.random_bases(rng, size), off)]
    return sc.Case(f"map_family_k{k}", genomes, [(q, r) for q in range(3) for r in range(3)], {(q, r) for q in (0, 1) for r in (0, 1)} | {(2, 2)})


RULES = dict(a=0, b=1, u=2, sh=3, dup=4)


@functools.lru_cache(maxsize=None)
def rules():
    """k 10, 120 kb, L 500, scale 4.  a: an ancestor; b: a 3 % copy; u: unrelated; sh: a with its half-fragments permuted (the even
    halves first, then the odd ones); dup: a[:20000] three times, then a[20000:60000]."""
    rng = np.random.default_rng(20261310)
    size, half = 120_000, 250
    a = sc.random_bases(rng, size)
    b = sc.substituted(rng, a)
    u = sc.random_bases(rng, size)
    halves = a.reshape(size // half, half)
    sh = np.concatenate([halves[0::2].ravel(), halves[1::2].ravel()])
    dup = np.concatenate([a[:20_000], a[:20_000], a[:20_000], a[20_000:60_000]])
    one = lambda s: (s, np.array([0, len(s)], dtype=np.uint64))
    R = RULES
    pairs = [(R["b"], R["a"]), (R["u"], R["a"]), (R["a"], R["u"]), (R["b"], R["sh"]), (R["dup"], R["a"]), (R["a"], R["dup"]), (R["a"], R["a"])]
    return sc.Case("map_rules", [one(a), one(b), one(u), one(sh), one(dup)], pairs)


@functools.lru_cache(maxsize=None)
def records(k):
    """sketch_k_cases.records(k) (0: several hundred short records, empty ones, N runs, lower case; 1: the same bases as one record) and
    2: the same bases in 7 records that end in the middle of a bin — a coordinate that counted the separator base of the packed stream
    would move a bin per 64 records in genome 0, and the windows with it."""
    base = skc.records(k)
    plain = base.genomes[1][0]
    genomes = list(base.genomes) + [(plain, sc.offsets(len(plain), 7, 13))]
    pairs = list(base.pairs) + [(1, 2), (2, 1), (0, 2), (2, 0), (2, 2)]
    case = sc.Case(f"map_records_k{k}", genomes, pairs)
    case.lengths = base.lengths
    return case


@functools.lru_cache(maxsize=None)
def edges():
    """k 12, L 256, scale 4.  0 ... 3: the first 255, 256, 257 and 512 bases of one sequence (nb = 1, 1, 2, 2); 4: its first 200 bases
    (a query of 0 fragments); 5: a query whose only fragment is all N."""
    rng = np.random.default_rng(20261320)
    s = sc.random_bases(rng, 512)
    one = lambda x: (x, np.array([0, len(x)], dtype=np.uint64))
    all_n = np.concatenate([np.full(256, ord("N"), dtype=np.uint8), s[:44]])
    genomes = [one(s[:255].copy()), one(s[:256].copy()), one(s[:257].copy()), one(s), one(s[:200].copy()), one(all_n)]
    pairs = [(q, r) for q in range(4) for r in range(4)] + [(4, 3), (5, 3), (3, 4), (3, 5), (4, 4), (5, 5)]
    return sc.Case("map_edges", genomes, pairs)


@functools.lru_cache(maxsize=None)
def repeats():
    """k 12, L 256, scale 1.  0: a reference with a 40-base unit 5 000 times in one block and 300 more copies scattered over 60 kb (every
    k-mer of the unit occurs in some 1 100 bins: more than a wave lists); 1: a query with the unit once; 2: with the unit 50 times."""
    rng = np.random.default_rng(20261330)
    unit = sc.random_bases(rng, 40)
    scattered = sc.random_bases(rng, 60_000)
    for at in np.sort(rng.choice(np.arange(0, 60_000 - 40, 200), size=300, replace=False)):
        scattered[at:at + 40] = unit
    ref = np.concatenate([sc.random_bases(rng, 1_003), np.tile(unit, 5_000), scattered])
    q1 = sc.random_bases(rng, 1_024); q1[300:340] = unit
    q50 = sc.random_bases(rng, 4_096); q50[500:2_500] = np.tile(unit, 50)
    one = lambda x: (x, np.array([0, len(x)], dtype=np.uint64))
    return sc.Case("map_repeats", [one(ref), one(q1), one(q50)], [(1, 0), (2, 0), (1, 2), (2, 1)])


CAPACITY_FRAG_LEN = 64
CAPACITY_LIMIT_BASES = MAX_BINS * CAPACITY_FRAG_LEN      # 524 288: the largest reference at frag_len 64


@functools.lru_cache(maxsize=None)
def capacity():
    """k 12, L 64, scale 16.  0: a reference of exactly 8 192 bins; 1: the same with one base more (8 193 bins: refused); 2: a 3 % copy of
    the last 20 000 bases of 0 (its fragments map into the last bins)."""
    rng = np.random.default_rng(20261340)
    big = sc.random_bases(rng, CAPACITY_LIMIT_BASES + 1)
    q = sc.substituted(rng, big[CAPACITY_LIMIT_BASES - 20_000:CAPACITY_LIMIT_BASES])
    one = lambda x: (x, np.array([0, len(x)], dtype=np.uint64))
    return sc.Case("map_capacity", [one(big[:CAPACITY_LIMIT_BASES].copy()), one(big), one(q)], [(2, 0), (2, 2)])


@functools.lru_cache(maxsize=None)
def wide():
    """k 12, L 70 000 (above 65 535: the mapping kernel's counters are 32 bits wide there), scale 16: 0 an ancestor of 150 kb in one
    record (2 fragments, 3 bins), 1 a 3 % copy, 2 unrelated; all 9 ordered pairs."""
    rng = np.random.default_rng(20261350)
    a = sc.random_bases(rng, 150_000)
    one = lambda x: (x, np.array([0, len(x)], dtype=np.uint64))
    return sc.Case("map_wide", [one(a), one(sc.substituted(rng, a)), one(sc.random_bases(rng, 150_000))], [(q, r) for q in range(3) for r in range(3)])


#   name: (case function, k, frag_len, scale, min_fraction)
SETS = {
    "family_k8": (functools.partial(family, 8), 8, 64, 4, 0.5),
    "family_k12": (functools.partial(family, 12), 12, 1000, 16, 0.2),
    "family_k12_L500": (functools.partial(family, 12), 12, 500, 16, 0.2),      # (the same genomes at another frag_len: the index is reused)
    "family_k16": (functools.partial(family, 16), 16, 3000, 16, 0.2),
    "rules": (rules, 10, 500, 4, 0.2),
    "records_k8": (functools.partial(records, 8), 8, 64, 16, 0.2),
    "records_k15": (functools.partial(records, 15), 15, 64, 16, 0.2),
    "edges": (edges, 12, 256, 4, 0.2),
    "repeats": (repeats, 12, 256, 1, 0.2),
    "wide": (wide, 12, 70_000, 16, 0.2),
    "capacity": (capacity, 12, CAPACITY_FRAG_LEN, 16, 0.2),
}


@functools.lru_cache(maxsize=None)
def _bins(name, g):
    fn, k, frag_len, scale, _ = SETS[name]
    seq, off = fn().genomes[g]
    return reference_bins(seq, off, k, frag_len, scale)


@functools.lru_cache(maxsize=None)
def _frags(name, g):
    fn, k, frag_len, scale, _ = SETS[name]
    seq, off = fn().genomes[g]
    return skc.genome_sketch(seq, off, k, frag_len=frag_len, scale=scale)


@functools.lru_cache(maxsize=None)
def answer(name, q, r, min_fraction=None):
    """mapped_pair of genomes q (query) and r (reference) of a set: (result, records, stats)."""
    _, k, _, _, mf = SETS[name]
    bins, nb = _bins(name, r)
    return mapped_pair(_frags(name, q)[1], bins, nb, k, mf if min_fraction is None else min_fraction)


def answers(name, pairs=None):
    return [answer(name, q, r) for q, r in (SETS[name][0]().pairs if pairs is None else pairs)]


def anywhere(name, q, r):
    """sketch_k_cases.sketch_pair (today's definition) of the same pair at the set's parameters."""
    _, k, _, _, mf = SETS[name]
    return skc.sketch_pair(_frags(name, q), _frags(name, r), k, mf)


def total_stats(names=None):
    tot = {}
    for name in (SETS if names is None else names):
        if name == "capacity":
            continue      # (sized for the limit, not for the rules)
        for _, _, st in answers(name):
            for key, v in st.items():
                tot[key] = tot.get(key, 0) + int(v)
    return tot
