"""CPU: the cases of tests/test_sketch_shapes_gpu.py (tests/sketch_cases.py) reach the launch paths they are written for, and the numpy
definition (oracle/sketch_oracle.py) gives them answers worth comparing.  Without this a later change to the generators, or to the
constants of pg_sketch_pairs, could turn the GPU tests into tests of the default path with nobody noticing: two all-zero tables are equal
too.

The two formulas are RESTATED here from the host code of pg_sketch_pairs (pyani_amd/csrc/pg_sketch.hip, "jobs: the pairs by query, up to
SK_REFS references per workgroup"):
    per_ref = max(n_frags, 1) * 4                       bytes of fragment counters per reference;  > 96 KiB: PG_E_CAPACITY
    g_max   = min(SK_REFS = 4, 96 KiB / per_ref)        references per workgroup
    LDS     = per_ref * (references of the job)         > 48 KiB: the hipFuncSetAttribute(..., 96 KiB) branch
and from build_sketch: grid = min(stream_len / 32 / 256 + 1, num_cu * 8) workgroups of 256 lanes, 32 start positions per lane."""
import math

import numpy as np
import pytest

from tests import sketch_cases as sc


def _g_max(n_frags):      # pg_sketch_pairs, restated (not imported from the helper: the helper is checked against it below)
    per_ref = max(n_frags, 1) * 4
    return min(4, (96 * 1024) // per_ref)


def _lds(n_frags, n_refs_in_job):
    return max(n_frags, 1) * 4 * n_refs_in_job


def test_helper_formulas_are_the_host_codes():
    for nf in (0, 1, 3072, 3073, 6144, 6145, 8192, 8193, 12288, 12289, 24576):
        assert sc.refs_per_job(nf) == _g_max(nf) and sc.per_ref_bytes(nf) == max(nf, 1) * 4
    assert sc.refs_per_job(24577) == 0 and 24577 * 4 > 96 * 1024 >= 24576 * 4
    assert [_g_max(nf) for nf in (6144, 6145, 8192, 8193, 12288, 12289, 24576)] == [4, 3, 3, 2, 2, 1, 1]
    assert _lds(3072, 4) == 48 * 1024 < _lds(3073, 4)
    assert sc.job_sizes(7000, 7) == [3, 3, 1] and sc.job_sizes(9000, 7) == [2, 2, 2, 1] and sc.job_sizes(14000, 3) == [1, 1, 1]


def test_mixed_case_sizes_reach_every_job_shape():
    case = sc.mixed()
    want_frags = {"small": 1_875, "lds96_4refs": 4_700, "3refs": 7_030, "2refs": 9_370, "1ref": 14_060}      # the issue's table (120 kb: 1 875)
    n_refs = {q: sum(1 for a, _ in case.pairs if a == q) for q in case.queries}
    assert sorted(case.queries) == sorted(case.ancestor.values()) and min(n_refs.values()) >= 7
    assert len(set(case.pairs)) == len(case.pairs) - 1                                      # one pair twice
    assert case.pairs != sorted(case.pairs)                                                 # shuffled
    shapes = set()
    for name, q in case.ancestor.items():
        seq, off = case.genomes[q]
        assert 2 <= len(off) - 1 <= 3 and all(int(b - a) % 32 for a, b in zip(off[:-1], off[1:])), name      # record lengths: no multiple of 32 (or 64)
        nf = case.fragments(q, 64)
        assert abs(nf - want_frags[name]) <= 20, (name, nf)
        g_max, big_lds = sc.MIXED_EXPECT[name]
        assert _g_max(nf) == g_max, (name, nf)
        jobs = sc.job_sizes(nf, n_refs[q])
        assert (max(_lds(nf, g) for g in jobs) > 48 * 1024) == big_lds, (name, nf, jobs)
        assert max(_lds(nf, g) for g in jobs) <= 96 * 1024
        shapes.add(tuple(jobs))
    assert (3, 3, 1) in shapes and (2, 2, 2, 1) in shapes and (1,) * 7 in shapes, shapes
    assert any(len(s) == 2 and s[0] == 4 for s in shapes)                                   # 4 + 3 (or 4 + 4: the query of the doubled pair)


def test_limit_production_and_record_cases_have_the_sizes_they_claim():
    lim = sc.limit()
    assert lim.fragments(0, 64) == 24_576 == sc.MAX_QUERY_FRAGMENTS and len(lim.genomes[0][0]) == 1_572_864 and len(lim.genomes[0][1]) == 2
    assert lim.fragments(1, 64) == 24_577 and len(lim.genomes[1][0]) == 1_572_864 + 64
    assert _g_max(24_576) == 1 and _lds(24_576, 1) == 96 * 1024 and 24_577 * 4 > 96 * 1024
    assert (lim.genomes[1][0][:1_572_864] == lim.genomes[0][0]).all()
    prod = sc.production()
    seq, off = prod.genomes[0]
    stream = len(seq) + len(off) - 2                                                        # one separator between records
    assert len(off) == 3 and stream > 256 * sc.SCAN_CHUNK_POSITIONS == 16_777_216          # a second grid-stride trip on 256 compute units
    nf = prod.fragments(0, sc.PROD_FRAG_LEN)
    assert 5_700 <= nf <= 5_900 and _g_max(nf) == 4 and _lds(nf, 3) > 48 * 1024            # three references in one job
    rec = sc.records()
    L = rec.lengths
    assert len(L) >= 300 and set(sc.RECORD_LENGTHS) <= set(L) and L[0] == 0 and L[-1] == 0
    assert rec.fragments(0, 64) == sum(n // 64 for n in L)
    seq, off = rec.genomes[0]
    starts = np.asarray(off[:-1], dtype=np.int64) + np.arange(len(L))                       # stream positions (a separator per boundary)
    chunks = np.unique(starts // 32)
    assert len(chunks) >= 200                                                               # a record boundary inside hundreds of chunks ...
    assert np.max(np.bincount((starts // 32).astype(np.int64))) >= 3                        # ... and three or more in one
    n_cross = 0
    for a, b in zip(off[:-1], off[1:]):
        r = bytes(seq[int(a):int(b)])
        for f in range(64, len(r) // 64 * 64, 64):
            n_cross += r[f - 1:f + 1] == b"NN"
    assert n_cross >= 8 and any(bytes(seq[int(a):int(b)]).islower() for a, b in zip(off[:-1], off[1:]) if b - a >= 200)
    assert bytes(rec.genomes[1][0]).upper() == bytes(rec.genomes[1][0]) and len(rec.genomes[1][1]) == 2


@pytest.mark.parametrize("scale", [1, 4])
def test_the_oracle_answers_of_the_mixed_call_are_not_vacuous(scale):
    case = sc.mixed()
    want = sc.oracle_pairs(sc.mixed, 64, scale, 0.2)
    strong, related, unrelated = sc.non_vacuity(case, want)
    assert related == 2 * len(case.queries) + ((case.pairs[-1]) in case.related) and unrelated >= 5 * len(case.queries)
    by = dict(zip(case.pairs, want))
    for name, q in case.ancestor.items():
        nf = case.fragments(q, 64)
        assert by[(q, q)][2:] == (nf, 0) and by[(q, q)][1] >= (nf if scale == 1 else 0.99 * nf)      # against itself (scale 1: every fragment)
        ani, matches, frags, status = by[(q, q + 1)]                                        # its 3 % copy
        assert frags == nf and status == 0 and matches >= 0.9 * nf and 0.95 < ani < 0.98, (name, scale, ani, matches, frags)


def test_the_oracle_answers_of_the_small_cases_are_not_vacuous():
    sc.non_vacuity(sc.limit(), sc.oracle_pairs(sc.limit, 64, 16, 0.2))
    sc.non_vacuity(sc.records(), sc.oracle_pairs(sc.records, 64, 16, 0.2))
    for frag_len, scale in sc.EDGE_PARAMS:
        want = sc.oracle_pairs(sc.edges, frag_len, scale, 0.2)
        if scale < 4096:
            sc.non_vacuity(sc.edges(), want)
        else:      # one k-mer in 4096: ~0.7 per fragment of 3000: most fragments lack the two hits a match needs, a few have them
            assert all(2 * m < f and f in (39, 40) for _, m, f, _ in want) and sum(m for _, m, _, _ in want) >= 10


def test_the_equality_pair_sits_exactly_on_the_min_fraction_comparison():
    """The definition compares in double: matches >= min_fraction * fragments.  For the chosen pair min_fraction = matches / fragments
    (one correctly rounded division) multiplies back to exactly `matches`, and the next double above it to more than `matches`: the two
    calls of the GPU test differ by one unit in the last place of min_fraction and in nothing else."""
    frag_len, scale = sc.EQUALITY_PARAMS
    q, r = sc.EQUALITY_PAIR
    _, matches, frags, _ = sc.oracle_pair(sc.edges, q, r, frag_len, scale, 0.2)
    assert 0 < matches < frags
    at = matches / frags
    above = float(np.nextafter(at, 2.0))
    assert at * float(frags) == float(matches) and above * float(frags) > float(matches) and above <= 1.0 and not math.isnan(above)
    assert sc.oracle_pair(sc.edges, q, r, frag_len, scale, at)[3] == 0
    assert sc.oracle_pair(sc.edges, q, r, frag_len, scale, above)[3] == 1
