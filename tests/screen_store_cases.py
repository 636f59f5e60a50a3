"""Hand-made search indexes for the tests of the index on disk and its shrinking (tests/test_screen_search_store_cpu.py,
tests/test_screen_search_store_gpu.py): an index in the build's layout from any list of k-mer sets and any cut of the
bins into slices, synthetic sampled k-mers found by brute force with the test-side hash (tests/screen_cases.py), and the single
corruptions of a sound index, each with the invariant it violates.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file, and nothing here imports pyani_amd.  Everything is computed once per
process and never written afterwards: corruptions() works on copies."""
import functools

import numpy as np

from tests import screen_cases as scr

NO_SLICE = 0xFFFFFFFF
THIRDS = (0, 1365, 2730, scr.N_BINS)


def mix(x):
    """The test-side hash on a COPY (it works in place on a uint64 array)."""
    return scr.mix32(np.array(x, dtype=np.uint64, copy=True).reshape(-1))


def bin_of(x, scale):
    return scr.bin_of(np.array(x, dtype=np.uint64, copy=True).reshape(-1), scale)


def sampled_kmers(rng, k, scale, count):
    """`count` distinct k-mers (< 4^k) that the sampling rule keeps under `scale`, by brute force."""
    out = np.zeros(0, dtype=np.uint64)
    while len(out) < count:
        x = rng.integers(0, 4 ** k, size=4 * count * scale, dtype=np.uint64)
        out = np.unique(np.concatenate([out, x[(mix(x) & np.uint64(scale - 1)) == 0]]))
    return rng.permutation(out)[:count]


def sliced_index(columns, k, scale, cuts=(0, scr.N_BINS), keys=0):
    """(shape, (kmer, start, member, slice_first, bin_slice)) of the index over the k-mer sets `columns` (one per genome), its slices the
    bin ranges [cuts[s], cuts[s + 1]): inside a slice the k-mers ascend, inside a k-mer the holders."""
    n = len(columns)
    allk = np.concatenate([np.asarray(c, dtype=np.uint64) for c in columns]) if n else np.zeros(0, np.uint64)
    owner = np.concatenate([np.full(len(c), g, dtype=np.uint32) for g, c in enumerate(columns)]) if n else np.zeros(0, np.uint32)
    n_slices = len(cuts) - 1 if len(allk) else 0
    bin_slice = np.full(scr.N_BINS, NO_SLICE, dtype=np.uint32)
    for s in range(n_slices):
        bin_slice[cuts[s]:cuts[s + 1]] = s
    sl = bin_slice[bin_of(allk, scale).astype(np.int64)] if len(allk) else np.zeros(0, np.uint32)
    order = np.lexsort((owner, allk, sl))
    allk, owner, sl = allk[order], owner[order], sl[order]
    head = np.ones(len(allk), dtype=bool)
    head[1:] = allk[1:] != allk[:-1]
    kmer = allk[head].astype(np.uint32)
    start = np.append(np.flatnonzero(head), len(allk)).astype(np.uint64)
    slice_first = np.searchsorted(sl[head], np.arange(n_slices + 1)).astype(np.uint64)
    return (n, k, scale, len(kmer), len(allk), n_slices, keys or len(allk)), (kmer, start, owner.astype(np.uint32), slice_first, bin_slice)


def columns_of(index):
    """The index read back as (k-mer -> tuple of holders), for comparisons that must not depend on the cut into slices."""
    _, (kmer, start, member, _, _) = index
    return {int(x): tuple(member[int(start[g]):int(start[g + 1])].tolist()) for g, x in enumerate(kmer)}


@functools.lru_cache(maxsize=None)
def built_index():
    """Four genomes over 40 synthetic k-mers in one slice, k = 16, scale = 16; genome 3 holds nothing."""
    rng = np.random.default_rng(20261022)
    pool = sampled_kmers(rng, 16, 16, 40)
    columns = [pool[rng.random(40) < p] for p in (0.7, 0.5, 0.3)] + [pool[:0]]
    return sliced_index(columns, 16, 16)


@functools.lru_cache(maxsize=None)
def three_slices():
    """Three genomes, three slices (thirds of the bins), k = 12, scale = 16: genome 1 holds every k-mer of the middle slice and nothing
    else, genomes 0 and 2 hold the rest (some of it both)."""
    rng = np.random.default_rng(20261023)
    pool = sampled_kmers(rng, 12, 16, 300)
    bins = bin_of(pool, 16)
    middle = (bins >= THIRDS[1]) & (bins < THIRDS[2])
    assert middle.sum() >= 20 and (bins < THIRDS[1]).sum() >= 20 and (bins >= THIRDS[2]).sum() >= 20
    rest = pool[~middle]
    return sliced_index([rest[rng.random(len(rest)) < 0.7], pool[middle], rest[rng.random(len(rest)) < 0.6]], 12, 16, THIRDS)


@functools.lru_cache(maxsize=None)
def corruptions():
    """{name: (shape, arrays, invariant)}: single corruptions of three_slices(); `invariant` is the key of
    pyani_amd.screen.SEARCH_INDEX_INVARIANTS that the validation must name FIRST."""
    shape, arrays = three_slices()
    n, k, scale, d, e, s, _ = shape
    kmer, start, member, slice_first, bin_slice = arrays
    wide = int(np.flatnonzero(np.diff(start.astype(np.int64)) >= 2)[0])      # a k-mer two genomes hold
    out = {}

    def case(name, invariant, which=None, change=None, new_shape=None):
        copy = [a.copy() for a in arrays]
        if change:
            change(copy[which])
        out[name] = (new_shape or shape, tuple(copy), invariant)

    def put(index, value):
        def change(a):
            a[index] = value
        return change

    case("member >= n", "member_range", 2, put(int(start[wide]) + 1, n))
    case("member far >= n", "member_range", 2, put(e - 1, 0xFFFFFFF0))
    case("descending holders", "member_order", 2, put(slice(int(start[wide]), int(start[wide]) + 2), member[int(start[wide]):int(start[wide]) + 2][::-1]))
    case("duplicate holder", "member_order", 2, put(int(start[wide]) + 1, member[int(start[wide])]))
    case("duplicate k-mer", "kmer_order", 0, put(1, kmer[0]))
    absent = next(int(x) for x in sampled_kmers(np.random.default_rng(3), k, scale, 400)
                  if int(bin_of([x], scale)[0]) >= THIRDS[2] and int(x) not in set(kmer.tolist()))
    case("k-mer in another slice's range", "kmer_slice", 0, put(0, absent))
    unsampled = next(x for x in range(int(kmer[2]) + 1, 4 ** k) if int(mix([x])[0]) & (scale - 1))
    case("unsampled k-mer", "kmer_sampled", 0, put(2, unsampled))
    case("k-mer >= 4^k", "kmer_range", 0, put(d - 1, 4 ** k + 5))
    case("start not increasing", "start_order", 1, put(3, start[2]))
    case("start descending far", "start_order", 1, put(4, 2 ** 40))
    case("start[D] != E", "start_end", 1, put(d, e - 1))
    case("start[0] != 0", "start0", 1, put(0, 1))
    case("slice_first descends", "slice_first", 3, put(1, slice_first[2] + 1))
    case("slice_first does not end at D", "slice_first", 3, put(s, d - 1))
    case("a bin names slice 7", "bin_slice", 4, put(9, 7))
    case("kmer = 7", "shape", new_shape=(n, 7, scale, d, e, s, e))
    case("scale = 24", "shape", new_shape=(n, k, 24, d, e, s, e))
    return out
