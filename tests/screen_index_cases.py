"""The input of the index path's test beyond the dense calls' limit (tests/test_screen_index_gpu.py) and its expected values, from the
building blocks of the statement (tests/screen_cases.genome_set, statement) — never an n x n array on the host.
TEST INFRASTRUCTURE ONLY: nothing under pyani_amd/ imports this file."""
import functools

import numpy as np

from tests import screen_cases as scr
from tests import sketch_cases as sc

BEYOND_N, BEYOND_BASES, BEYOND_PARAMS = 8200, 48, (16, 1)
BEYOND_B_HOLDERS = (0, 8191, 8192, 8199)      # either side of the old limit, and both ends
BEYOND_PLAIN = (1, 4096, 8193)                # genomes that hold motif A only: the other kind of genome


@functools.lru_cache(maxsize=None)
def beyond():
    """8200 genomes of 48 bases.  Motif A (24 bases: 9 16-mers) is in ALL of them: groups of 8200 members.  Motif B (24 bases) stands in
    place of the random rest in the four BEYOND_B_HOLDERS only.  A comes first in the even genomes and last in the odd ones.
    The motif and the rest are two RECORDS of 24 bases: no window spans their junction.  In one record the k-mers with 15, 14, ... bases
    of A and 1, 2, ... random ones would be shared by a quarter, a sixteenth, ... of the genomes, and among 3 x 10^7 pairs some with
    nothing but A in common would share more than two B holders do: no threshold would separate them."""
    rng = np.random.default_rng(20261906)
    ma, mb = sc.random_bases(rng, 24), sc.random_bases(rng, 24)
    off = np.array([0, BEYOND_BASES // 2, BEYOND_BASES], dtype=np.uint64)
    genomes = []
    for g in range(BEYOND_N):
        rest = mb if g in BEYOND_B_HOLDERS else sc.random_bases(rng, 24)
        genomes.append((np.concatenate([ma, rest] if g % 2 == 0 else [rest, ma]), off))
    return genomes


@functools.lru_cache(maxsize=None)
def beyond_sets():
    """(S(g) of every genome, all of them concatenated, the owner of each entry)."""
    k, scale = BEYOND_PARAMS
    sets = [scr.genome_set(s, o, k, scale) for s, o in beyond()]
    return sets, np.concatenate(sets), np.concatenate([np.full(len(x), g, dtype=np.int64) for g, x in enumerate(sets)])


@functools.lru_cache(maxsize=None)
def beyond_sizes():
    out = np.array([len(x) for x in beyond_sets()[0]], dtype=np.uint32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def beyond_rows(r0, r1):
    """The rows [r0, r1) of the matrix, uint32[r1 - r0, n]: every k-mer held by two or more genomes adds one to the cells (a, b) of its
    holders a in [r0, r1) and b anywhere; the diagonal = sizes."""
    _, allk, owner = beyond_sets()
    _, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
    multi = cnt >= 2                                   # (a few dozen k-mers: the motifs' and the chance ones)
    col = np.cumsum(multi) - 1
    keep = multi[inv]
    inc = np.zeros((BEYOND_N, int(multi.sum())), dtype=np.float64)      # the statement's incidence, genome x shared k-mer (counts below 2^53: exact)
    inc[owner[keep], col[inv[keep]]] = 1.0
    out = np.rint(inc[r0:r1] @ inc.T).astype(np.uint32)
    rows = np.arange(r0, r1)
    out[rows - r0, rows] = beyond_sizes()[r0:r1]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def beyond_handful():
    """(genomes of the handful, sizes, shared) by the STATEMENT itself on the B holders and three plain genomes: shared[a][b] depends on a
    and b alone, so these are the matrix's cells of those genomes."""
    k, scale = BEYOND_PARAMS
    who = list(BEYOND_B_HOLDERS) + list(BEYOND_PLAIN)
    sizes, shared = scr.statement([beyond()[g] for g in who], k, scale)
    return who, sizes, shared


def beyond_threshold():
    """(t, the largest identity of a pair that shares motif A only, the smallest of two B holders): t halfway between the two."""
    who, sizes, shared = beyond_handful()
    ident = scr.identity_of(sizes, shared, BEYOND_PARAMS[0])
    nb = len(BEYOND_B_HOLDERS)
    idx = np.arange(len(who))
    off_diag = idx[:, None] != idx[None, :]
    both_b = (idx[:, None] < nb) & (idx[None, :] < nb) & off_diag
    a_only = float(ident[off_diag & ~both_b].max())
    a_and_b = float(ident[both_b].min())
    return (a_only + a_and_b) / 2.0, a_only, a_and_b
