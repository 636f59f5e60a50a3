"""run_screen_search and run_screen_gather with db_batch= (pyani_amd/subcmd_search.py, subcmd_gather.py): the collection
goes through the genome store a few files at a time — the first batch indexed, every later one added to the resident index, the store
cleared after each — and the run must give what the run without db_batch gives: the same arrays, frames and files, byte for byte."""
import numpy as np
import pytest
from pandas.testing import assert_frame_equal

from tests import screen_cases as scr
from tests import screen_gather_cases as sgc
from tests import screen_search_cases as ssx

pytestmark = pytest.mark.gpu

K, SCALE, NEED = 16, 16, 10


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """(db, search queries, gather queries): the family's db genomes (5 files: batches of 2 + 2 + 1), its search queries, the mixture."""
    from pyani_amd import synth
    db, sq, gq = (tmp_path_factory.mktemp(x) for x in ("add_db", "add_search_queries", "add_gather_queries"))
    fam = scr.family()
    for g in ssx.FAMILY_DB:
        synth.write_fasta(db / f"fam{g}.fna", *fam[g], f"fam{g}")
    for g in ssx.FAMILY_QUERIES:
        synth.write_fasta(sq / f"query{g}.fna", *fam[g], f"query{g}")
    for name, (seq, off) in zip(("mix", "copy"), sgc.mixture_queries()):
        synth.write_fasta(gq / f"{name}.fna", seq, off, name)
    return db, sq, gq


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


def _same_arrays(got, want, names):
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
        else:
            assert g == w, name


def _same_files(got, want):
    assert [p.name for p in got] == [p.name for p in want] and len(want) == 2
    for g, w in zip(got, want):
        assert g.read_bytes() == w.read_bytes() and len(w.read_bytes()) > 0, g.name


def test_search_in_batches_equals_the_plain_run(eng, dirs, tmp_path):
    from pyani_amd.subcmd_search import run_screen_search
    db, sq, _ = dirs
    args = dict(min_identity=0.8, kmer=K, scale=SCALE, top=2, write_output=True, engine=eng)
    plain = run_screen_search(db, sq, tmp_path / "plain", **args)
    qs, ds, hits = ssx.block("family", K, SCALE, ssx.FAMILY_QUERIES, ssx.FAMILY_DB)
    assert (plain.hits.db_sizes == ds).all() and (plain.hits.query_sizes == qs).all() and 0 < len(plain.hits.a) < hits.size
    for batch in (2, 1, np.int64(3), 5, 99):
        run = run_screen_search(db, sq, tmp_path / f"batch{batch}", db_batch=batch, **args)
        assert eng.genome_count() == 0 and run.exact is None
        with pytest.raises(Exception):      # the run left no index behind
            eng.screen_search_count([])
        assert run.db_lengths == plain.db_lengths and list(run.db_lengths) == list(plain.db_lengths) and run.query_lengths == plain.query_lengths
        for got, want in ((run.hits, plain.hits), (run.best, plain.best)):
            _same_arrays(got, want, ("query_labels", "db_labels", "options", "query_sizes", "db_sizes", "a", "b", "shared"))
        assert_frame_equal(run.frame, plain.frame, check_exact=True)
        _same_files(run.written, plain.written)


def test_gather_in_batches_equals_the_plain_run(eng, dirs, tmp_path):
    from pyani_amd.subcmd_gather import run_screen_gather
    db, _, gq = dirs
    args = dict(min_unique=NEED, kmer=K, scale=SCALE, write_output=True, engine=eng)
    plain = run_screen_gather(db, gq, tmp_path / "plain", **args)
    fam = scr.family()
    queries = sgc.mixture_queries()
    want = sgc.gather_genomes([queries[1], queries[0]], [fam[g] for g in ssx.FAMILY_DB], K, SCALE, NEED)      # file order: copy.fna, mix.fna
    sgc.same_rows((plain.result.query, plain.result.db, plain.result.unique, plain.result.total), want, "plain")
    assert len(want.query) >= 3
    for batch in (2, 1, 3):
        run = run_screen_gather(db, gq, tmp_path / f"batch{batch}", db_batch=batch, **args)
        assert eng.genome_count() == 0 and run.exact is None
        assert run.db_lengths == plain.db_lengths and list(run.db_lengths) == list(plain.db_lengths) and run.query_lengths == plain.query_lengths
        _same_arrays(run.result, plain.result, plain.result._fields)
        assert_frame_equal(run.frame, plain.frame, check_exact=True)
        assert_frame_equal(run.summary, plain.summary, check_exact=True)
        _same_files(run.written, plain.written)


def test_db_batch_refusals(eng, dirs):
    from pyani_amd.subcmd_gather import run_screen_gather
    from pyani_amd.subcmd_search import run_screen_search
    db, sq, gq = dirs
    eng.clear_genomes()
    for run, q, args in ((run_screen_search, sq, {"min_identity": 0.8}), (run_screen_gather, gq, {"min_unique": NEED})):
        with pytest.raises(ValueError, match="exact="):
            run(db, q, db_batch=2, exact="anim", engine=eng, kmer=K, scale=SCALE, **args)
        for bad in (0, True, 2.0, "2"):
            with pytest.raises(ValueError, match="db_batch must be an integer >= 1"):
                run(db, q, db_batch=bad, engine=eng, **args)
    assert eng.genome_count() == 0
    held = eng.add_genome(*scr.family()[0])      # the run does not own the store: nothing is read, nothing is cleared
    try:
        for run, q, args in ((run_screen_search, sq, {"min_identity": 0.8}), (run_screen_gather, gq, {"min_unique": NEED})):
            with pytest.raises(ValueError, match="store is empty"):
                run(db, q, db_batch=2, engine=eng, kmer=K, scale=SCALE, **args)
            with pytest.raises(ValueError, match="exact="):
                run(db, q, db_batch=2, exact="anim", engine=eng, kmer=K, scale=SCALE, **args)
            assert eng.genome_count() == 1 and held == 0
    finally:
        eng.clear_genomes()
