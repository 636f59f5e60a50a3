"""GPU (through the C ABI): the launch paths of the sketch mode that genomes of a few hundred fragments never take (pg_sketch_pairs and
sketch_scan_kernel, pyani_amd/csrc/pg_sketch.hip) against the numpy definition (oracle/sketch_oracle.py) — matches, fragments and status
equal, the ANI estimate bit-equal, error codes equal; no tolerance anywhere.  The cases and their expected values live in
tests/sketch_cases.py; tests/test_sketch_shapes_cpu.py holds them on the paths named here.

    test_mixed_call_*            > 48 KiB of dynamic LDS; 4, 3, 2 and 1 references per workgroup (jobs of 3 + 3 + 1, 2 + 2 + 2 + 1, 1 x 7);
                                 the hits[g * nf + fr] layout and J.out[] of split queries; scale 1 (log2_scale 0) and 4
    test_capacity_limit_*        24 576 fragments accepted (96 KiB for one reference), 24 577 refused, the engine afterwards
    test_production_parameters_* the second grid-stride trip of sketch_scan_kernel; frag_len 3000 with > 48 KiB of LDS
    test_records_inside_*        rec_of / rec_lo / rec_hi / n_full with several records in one 32-position chunk
    test_parameter_edges_*       scale 1 and 4096 (the table-size floor), frag_len 64 and 65, min_fraction at equality, PG_E_ARG
    test_cache_*                 rebuilds on a parameter change, ids reused after clear_genomes, genomes added after sketches exist"""
import numpy as np
import pytest

from tests import sketch_cases as sc

pytestmark = pytest.mark.gpu


def _engine_with(genomes):
    from pyani_amd.engine import Engine
    eng = Engine(0)
    ids = [eng.add_genome(s, o) for s, o in genomes]
    assert ids == list(range(len(genomes)))
    return eng


def _call(eng, pairs, frag_len, scale, min_fraction=0.2):
    return eng.sketch_pairs([q for q, _ in pairs], [r for _, r in pairs], frag_len=frag_len, scale=scale, min_fraction=min_fraction)


@pytest.fixture(scope="module")
def mixed_eng():
    eng = _engine_with(sc.mixed().genomes)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def edges_eng():
    eng = _engine_with(sc.edges().genomes)
    yield eng
    eng.close()


@pytest.mark.parametrize("scale", [1, 4])
def test_mixed_call_of_every_job_shape_equals_the_definition(mixed_eng, scale):
    case = sc.mixed()
    want = sc.oracle_pairs(sc.mixed, 64, scale, 0.2)
    sc.non_vacuity(case, want)
    res = _call(mixed_eng, case.pairs, 64, scale)
    sc.assert_records_equal(res, want, ("mixed", scale))
    assert res[-1].tobytes() == res[3].tobytes()                                            # the pair that is in the call twice
    # a result does not depend on how the call was cut into jobs: every pair alone (one job of one reference) gives the same bytes
    for k, pair in enumerate(case.pairs):
        alone = _call(mixed_eng, [pair], 64, scale)
        assert alone.tobytes() == res[k:k + 1].tobytes(), (scale, k, pair, alone, res[k])


def test_capacity_limit_the_largest_query_and_the_refusal_above_it():
    from pyani_amd import _lib
    case = sc.limit()
    assert case.fragments(0, 64) == 24_576 and case.fragments(1, 64) == 24_577
    want = sc.oracle_pairs(sc.limit, 64, 16, 0.2)
    sc.non_vacuity(case, want)
    eng = _engine_with(case.genomes)
    try:
        before = _call(eng, case.pairs, 64, 16)                                             # 24 576 fragments as the query; 24 577 as a reference
        sc.assert_records_equal(before, want, "limit")
        assert int(before[0]["fragments"]) == 24_576
        for pairs in ([(1, 0)], [(2, 2), (1, 2), (0, 0)]):                                  # 24 577 fragments as the query: alone, and amid valid pairs
            with pytest.raises(_lib.PyaniGpuError) as ei:
                _call(eng, pairs, 64, 16)
            assert ei.value.code == _lib.PG_E_CAPACITY
        after = _call(eng, case.pairs, 64, 16)
        assert after.tobytes() == before.tobytes()
        assert int(_call(eng, [(1, 1)], 3000, 16)[0]["fragments"]) == (1_572_864 + 64) // 3000      # (the same genome is a fine query at another frag_len)
    finally:
        eng.close()


def test_production_parameters_second_grid_stride_trip():
    """A 17.5 Mb genome at frag_len 3000, scale 64.  SKIPPED (with the reason printed) only on a device whose scan grid covers the whole
    stream in one trip: num_cu * 8 workgroups * 256 lanes * 32 positions >= the stream length (more than 267 compute units; MI355X: 256)."""
    import torch
    case = sc.production()
    seq, off = case.genomes[0]
    stream = len(seq) + len(off) - 2
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if num_cu * sc.SCAN_CHUNK_POSITIONS >= stream:
        print(f"skipped: {num_cu} compute units scan {num_cu * sc.SCAN_CHUNK_POSITIONS} positions in one trip, the stream has {stream}")
        pytest.skip(f"the scan grid of {num_cu} compute units covers the {stream}-position stream in one trip")
    want = sc.oracle_pairs(sc.production, sc.PROD_FRAG_LEN, sc.PROD_SCALE, 0.1)
    sc.non_vacuity(case, want)
    eng = _engine_with(case.genomes)
    try:
        res = _call(eng, case.pairs, sc.PROD_FRAG_LEN, sc.PROD_SCALE, 0.1)
    finally:
        eng.close()
    sc.assert_records_equal(res, want, "production")
    assert int(res[0]["fragments"]) == case.fragments(0, 3000) > 3072 and int(res[0]["matches"]) == int(res[0]["fragments"])


def test_records_inside_one_chunk_equal_the_definition():
    case = sc.records()
    want = sc.oracle_pairs(sc.records, 64, 16, 0.2)
    sc.non_vacuity(case, want)
    eng = _engine_with(case.genomes)
    try:
        res = _call(eng, case.pairs, 64, 16)
        sc.assert_records_equal(res, want, "records")
        assert int(res[0]["fragments"]) == int(res[1]["fragments"]) == sum(n // 64 for n in case.lengths)
        for scale in (1, 4):                                                                # every k-mer sampled: every position of every record counts
            sc.assert_records_equal(_call(eng, case.pairs, 64, scale), sc.oracle_pairs(sc.records, 64, scale, 0.2), ("records", scale))
    finally:
        eng.close()


def test_parameter_edges_equal_the_definition(edges_eng):
    case = sc.edges()
    for frag_len, scale in sc.EDGE_PARAMS:
        for minfrac in (0.2, 0.0, 1.0) if (frag_len, scale) == (64, 16) else (0.2,):
            want = sc.oracle_pairs(sc.edges, frag_len, scale, minfrac)
            sc.assert_records_equal(_call(edges_eng, case.pairs, frag_len, scale, minfrac), want, (frag_len, scale, minfrac))
    assert len(_call(edges_eng, [], 3000, 16)) == 0                                         # an empty pair list


def test_min_fraction_comparison_at_equality(edges_eng):
    frag_len, scale = sc.EQUALITY_PARAMS
    pair = sc.EQUALITY_PAIR
    r = _call(edges_eng, [pair], frag_len, scale, 0.0)[0]
    matches, frags = int(r["matches"]), int(r["fragments"])
    assert (matches, frags) == sc.oracle_pair(sc.edges, *pair, frag_len, scale, 0.2)[1:3] and 0 < matches < frags
    at = matches / frags
    above = float(np.nextafter(at, 2.0))
    on = _call(edges_eng, [pair], frag_len, scale, at)
    over = _call(edges_eng, [pair], frag_len, scale, above)
    assert int(on[0]["status"]) == 0 and float(on[0]["ani"]).hex() == float(r["ani"]).hex()
    assert int(over[0]["status"]) == 1 and float(over[0]["ani"]) == 0.0 and int(over[0]["matches"]) == matches
    sc.assert_records_equal(on, [sc.oracle_pair(sc.edges, *pair, frag_len, scale, at)], "at equality")
    sc.assert_records_equal(over, [sc.oracle_pair(sc.edges, *pair, frag_len, scale, above)], "one ulp above")


def test_bad_arguments_are_refused(edges_eng):
    from pyani_amd import _lib
    good = dict(frag_len=3000, scale=16, min_fraction=0.2)
    before = edges_eng.sketch_pairs([0], [1], **good)
    for bad in (dict(frag_len=63), dict(scale=0), dict(scale=8192), dict(min_fraction=-0.1), dict(min_fraction=1.5), dict(min_fraction=float("nan"))):
        with pytest.raises(_lib.PyaniGpuError) as ei:
            edges_eng.sketch_pairs([0], [1], **dict(good, **bad))
        assert ei.value.code == _lib.PG_E_ARG, bad
    n = edges_eng.genome_count()
    for q, r in (([n], [0]), ([0], [n]), ([-1], [0]), ([0, 0], [1, n])):
        with pytest.raises(_lib.PyaniGpuError) as ei:
            edges_eng.sketch_pairs(q, r, **good)
        assert ei.value.code == _lib.PG_E_ARG, (q, r)
    with pytest.raises(ValueError):
        edges_eng.sketch_pairs([0, 1], [1], **good)
    assert edges_eng.sketch_pairs([0], [1], **good).tobytes() == before.tobytes()


def test_cache_rebuilds_when_the_parameters_change_and_change_back(edges_eng):
    case = sc.edges()
    first = _call(edges_eng, case.pairs, 3000, 16)
    other = _call(edges_eng, case.pairs[:6], 64, 4)                                         # rebuilds genomes 0 ... 3 (0 and 1 as queries); the rest keep (3000, 16)
    third = _call(edges_eng, case.pairs, 3000, 16)
    assert third.tobytes() == first.tobytes()
    sc.assert_records_equal(other, sc.oracle_pairs(sc.edges, 64, 4, 0.2, case.pairs[:6]), "(64, 4) between two (3000, 16) calls")
    assert first.tobytes() != _call(edges_eng, case.pairs, 64, 4).tobytes()


def test_cache_is_dropped_with_the_genomes_and_extended_by_later_ones():
    import sketch_oracle as so
    case = sc.edges()
    new, new_copy = sc.replacement()
    pairs = [(0, 0), (0, 1), (1, 0)]
    eng = _engine_with(case.genomes[:2])
    try:
        old = _call(eng, pairs, 64, 16)
        sc.assert_records_equal(old, sc.oracle_pairs(sc.edges, 64, 16, 0.2, pairs), "before later genomes")
        # genomes added after sketches exist (the arena is uploaded again): ids 2, 3 = the case's 2, 3
        assert [eng.add_genome(*g) for g in case.genomes[2:]] == [2, 3]
        mixed_pairs = [(2, 0), (0, 2), (3, 1), (2, 2), (1, 3)]
        got = _call(eng, pairs + mixed_pairs, 64, 16)
        assert got[:len(pairs)].tobytes() == old.tobytes()
        sc.assert_records_equal(got[len(pairs):], sc.oracle_pairs(sc.edges, 64, 16, 0.2, mixed_pairs), "old and new genomes")
        # clear_genomes(), then OTHER genomes under the ids 0 and 1: a sketch kept from before would answer for the old genome
        eng.clear_genomes()
        assert [eng.add_genome(*new), eng.add_genome(*new_copy)] == [0, 1]
        sk = [so.genome_sketch(s, o, frag_len=64, scale=16) for s, o in (new, new_copy)]
        want = [so.sketch_pair(sk[q], sk[r], 0.2) for q, r in pairs]
        assert want[1][3] == 0 and want[1][:3] != sc.oracle_pair(sc.edges, 0, 1, 64, 16, 0.2)[:3]
        sc.assert_records_equal(_call(eng, pairs, 64, 16), want, "same ids, other genomes")
    finally:
        eng.close()
