"""The profile's cases and an INDEPENDENT brute force of its definition in Python dicts and sets (tests/test_screen_profile_cpu.py,
tests/test_screen_profile_gpu.py).  The hand-made indexes come from tests/screen_store_cases.sliced_index: a few hundred
synthetic sampled k-mers whose holders are chosen so that every tier, every tier edge and every kind of cell occurs.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file.  Everything is computed once per process and never written
afterwards."""
import functools
from collections import Counter

import numpy as np

from tests import screen_store_cases as ssc

TIER_SETTINGS = ((0, 0), (0, 64), (1, 1), (4, 32), (8, 64), (None, None))      # (lane_limit, wave_limit); None: the default
TIER_HOLDERS = (1, 2, 4, 5, 8, 9, 63, 64, 65, 129, 3000)                # lane_limit and lane_limit + 1 for the limits 1, 4 and 8 (the default); the wave's 64
TIERS_N = 3001


def index_of(holders, n, k=16, scale=16, cuts=(0, 4096), seed=1):
    """The index in which synthetic k-mer i is held by the genomes holders[i] (each a non-empty collection of genomes below n)."""
    pool = ssc.sampled_kmers(np.random.default_rng(seed), k, scale, len(holders))
    columns = [[] for _ in range(n)]
    for x, hs in zip(pool.tolist(), holders):
        for g in sorted(set(int(v) for v in hs)):
            columns[g].append(x)
    return ssc.sliced_index([np.array(c, dtype=np.uint64) for c in columns], k, scale, cuts)


def groups_label(n, groups):
    """label int32[n]: every listed group a cluster named by its smallest member, every other genome a singleton."""
    label = np.arange(n, dtype=np.int32)
    for g in groups:
        label[np.asarray(list(g), dtype=np.int64)] = min(g)
    return label


def brute(index, label, core_need, shell_need, marker_min_size):
    """The definition over a hand-made index: brute_of with the index's k-mers in its own order and their holders read back."""
    shape, (kmer, _, _, _, _) = index
    return brute_of(kmer.tolist(), ssc.columns_of(index), shape[0], label, core_need, shell_need, marker_min_size)


def brute_of(kmers, holders, n, label, core_need, shell_need, marker_min_size):
    """The definition, cell by cell, for the k-mers `kmers` in index order and holders = {k-mer: its holders}: (genome arrays, cluster
    arrays, spectrum, off, marker arrays) in the statement's layout."""
    label = [int(x) for x in label]
    size = Counter(label)
    names = sorted(size)
    off, total = {}, 0
    for c in names:
        off[c] = total
        total += size[c]
    g_held, g_core, g_private, g_alone, g_foreign = ([0] * n for _ in range(5))
    c_kmers, c_core, c_soft, c_shell, c_private, c_marker = ([0] * n for _ in range(6))
    spectrum = [0] * n
    markers = []
    for position, x in enumerate(kmers):
        hs = set(holders[x])
        assert hs
        for c in sorted({label[v] for v in hs}):
            inside = {v for v in hs if label[v] == c}
            occ = len(inside)
            soft = occ >= int(core_need[c])
            private = inside == hs
            c_kmers[c] += 1
            c_core[c] += occ == size[c]
            c_soft[c] += soft
            c_shell[c] += (not soft) and occ >= int(shell_need[c])
            c_private[c] += private
            c_marker[c] += private and soft
            spectrum[off[c] + occ - 1] += 1
            if private and soft and size[c] >= marker_min_size:
                markers.append((c, position, x, occ))
            for v in inside:
                g_held[v] += 1
                g_core[v] += soft
                g_private[v] += private
                g_alone[v] += occ == 1
                g_foreign[v] += occ == 1 and len(hs) > 1
    markers.sort(key=lambda m: (m[0], m[1]))
    u32, u64 = (lambda a: np.array(a, dtype=np.uint32)), (lambda a: np.array(a, dtype=np.uint64))
    return ((u32(g_held), u32(g_core), u32(g_private), u32(g_alone), u32(g_foreign)),
            (u32([size.get(c, 0) for c in range(n)]), u64(c_kmers), u64(c_core), u64(c_soft), u64(c_shell), u64(c_private), u64(c_marker)),
            u64(spectrum), np.array([off.get(c, 0) for c in range(n)], dtype=np.int64),
            (np.array([m[0] for m in markers], dtype=np.int32), u32([m[2] for m in markers]), u32([m[3] for m in markers])))


def same(got, want):
    """Every array of two results equal, types included; returns the name of the first that differs, or None."""
    flat = lambda r: list(r[0]) + list(r[1]) + [r[2], r[3]] + list(r[4])      # noqa: E731
    names = ["held", "core_held", "private_held", "alone", "foreign", "size", "kmers", "core", "soft", "shell", "private", "marker", "spectrum", "off",
             "marker_cluster", "marker_kmer", "marker_occ"]
    for name, a, b in zip(names, flat(got), flat(want)):
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            return name
    return None


# ---- tier edges ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiers_index():
    """3001 genomes in three slices.  For every h of TIER_HOLDERS three k-mers: held by the genomes 0 ... h - 1 (the 129-holder one covers
    the clusters of 64 and of 65 of the partition "blocks" exactly), by a random h of them, and by every (n // h)-th; 120 more with one
    random holder each.  Genome 3000 holds little, several genomes nothing."""
    rng = np.random.default_rng(20261101)
    n = TIERS_N
    holders = []
    for h in TIER_HOLDERS:
        holders.append(range(h))
        holders.append(rng.choice(n, size=h, replace=False).tolist())
        holders.append((np.arange(h) * (n // h)).tolist())
    holders += [[int(rng.integers(0, n))] for _ in range(120)]
    return index_of(holders, n, cuts=ssc.THIRDS, seed=11)


@functools.lru_cache(maxsize=None)
def tiers_partitions():
    """name -> label over the 3001 genomes: members interleaved by index; one cluster of all; all singletons; a cluster of 64 and one of
    65 side by side (the rest interleaved by 7 behind them)."""
    n = TIERS_N
    v = np.arange(n, dtype=np.int32)
    blocks = np.where(v < 64, 0, np.where(v < 129, 64, 129 + (v - 129) % 7)).astype(np.int32)
    return {"mod7": (v % 7).astype(np.int32), "one": np.zeros(n, dtype=np.int32), "singletons": v.copy(), "blocks": blocks}


# ---- marker logic --------------------------------------------------------------------------------------------------------------------------
MARKER_N = 64
MARKER_GROUPS = (range(0, 20), range(20, 40), range(40, 60), range(60, 63))      # A, B, C of 20, D of 3; genome 63 a singleton


@functools.lru_cache(maxsize=None)
def marker_index():
    """The four directed cells of cluster A (its core_need is 19 at 0.95) and what the list's order needs: k-mer 0 the whole of A (marker,
    core); 1 the whole of A and genome 20 (core, not private); 2 A without genome 19 (private, soft iff core_need <= 19); 3 genome 5 of A
    and members of B, C and D (foreign for genome 5); then whole-cluster k-mers of B, D, the singleton, C, A, B again — markers whose
    index positions do not follow their clusters — and a shell k-mer of B."""
    a, b, c, d = (list(g) for g in MARKER_GROUPS)
    holders = [a, a + [20], a[:19], [5, 21, 22, 41, 60], b, d, [63], c, a, b, b[:4], c[:19], [63], d[:2]]
    return index_of(holders, MARKER_N, k=12, scale=16, seed=12)


def marker_label():
    return groups_label(MARKER_N, MARKER_GROUPS)


# ---- slices and empties ----------------------------------------------------------------------------------------------------------------------
def small_cases():
    """[(name, index, label)]: the three-slice index of the store's tests under three partitions, its four-genome index whose last genome
    holds nothing, and one genome alone."""
    one = index_of([[0]] * 7, 1, k=12, scale=16, seed=13)
    return [("three_slices singletons", ssc.three_slices(), np.arange(3, dtype=np.int32)),
            ("three_slices one", ssc.three_slices(), np.zeros(3, dtype=np.int32)),
            ("three_slices 0+2", ssc.three_slices(), np.array([0, 1, 0], dtype=np.int32)),
            ("built_index empty genome", ssc.built_index(), np.array([0, 0, 2, 3], dtype=np.int32)),
            ("built_index empty member", ssc.built_index(), np.array([0, 1, 1, 1], dtype=np.int32)),
            ("one genome", one, np.zeros(1, dtype=np.int32))]


def all_cases():
    """Every small case of both test files: (name, index, label)."""
    out = small_cases()
    out += [(f"tiers {name}", tiers_index(), label) for name, label in tiers_partitions().items()]
    out.append(("marker", marker_index(), marker_label()))
    return out


# ---- through the real scan -----------------------------------------------------------------------------------------------------------------------
def genome_kmers(seq, rec_off, k, scale):
    """S(g) with the k-mers' own VALUES, sorted: the distinct sampled canonical k-mers of every record.  (tests/screen_cases.genome_set
    gives the same sets under a bijection — its hash works in place on the k-mers before they are selected — which is all that sizes and
    shared counts need; the profile lists values, so the hash runs on a copy here.)"""
    from tests import sketch_k_cases as skc
    out = [np.zeros(0, dtype=np.uint64)]
    for r in range(len(rec_off) - 1):
        _, km = skc.record_kmers(np.asarray(seq[int(rec_off[r]):int(rec_off[r + 1])]), k)
        out.append(km[(ssc.mix(km) & np.uint64(scale - 1)) == 0])
    return np.unique(np.concatenate(out))


# ---- the scale of the relabel ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def million_index():
    """2^20 genomes: one k-mer held by all of them, 2^10 held by 1024 consecutive genomes each; one slice.  Made array by array (a list of
    2^20 columns would take sliced_index seconds)."""
    n, k, scale = 1 << 20, 16, 16
    pool = np.sort(ssc.sampled_kmers(np.random.default_rng(14), k, scale, 1025))
    kmer = pool.astype(np.uint32)
    h = np.full(1025, 1024, dtype=np.int64)
    everyone = 517
    h[everyone] = n
    start = np.concatenate([[0], np.cumsum(h)]).astype(np.uint64)
    blocks = iter(range(1024))
    member = np.concatenate([np.arange(n, dtype=np.uint32) if i == everyone else np.arange(1024, dtype=np.uint32) + np.uint32(1024 * next(blocks))
                             for i in range(1025)])
    bin_slice = np.zeros(4096, dtype=np.uint32)
    return (n, k, scale, 1025, len(member), 1, len(member)), (kmer, start, member, np.array([0, 1025], dtype=np.uint64), bin_slice)
