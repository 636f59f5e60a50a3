"""run_screen_search (pyani_amd/subcmd_search.py) on the genomes of the screened runs (tests/test_run_screened_gpu.py): the six as the
collection, family A as the queries — so every query meets itself in the collection, its two relatives, and nothing of family B."""
import numpy as np
import pandas as pd
import pytest

from tests import screen_select_cases as ssc
from tests.test_run_screened_gpu import STEMS, eng, indir      # noqa: F401 — the fixtures of the screened runs

pytestmark = pytest.mark.gpu

QUERIES = STEMS[:3]
KEPT = [(q, d) for q in QUERIES for d in STEMS[:3]]      # row-major: every query against family A, itself included


@pytest.fixture(scope="module")
def query_dir(tmp_path_factory):
    from pyani_amd import synth
    d = tmp_path_factory.mktemp("search_queries")
    for stem, (seq, off) in zip(QUERIES, ssc.run_genomes()):
        synth.write_fasta(d / f"{stem}.fna", seq, off, stem)
    return d


def _read(path):
    return pd.read_csv(path, sep="\t", float_precision="round_trip")


def _same_table(tab, frame):
    assert list(tab.columns) == list(frame.columns) and len(tab) == len(frame)
    for c in frame.columns:
        if frame[c].dtype == object:
            assert list(tab[c]) == list(frame[c]), c
        else:
            assert np.array_equal(tab[c].to_numpy(dtype=np.float64), frame[c].to_numpy(dtype=np.float64), equal_nan=True), c


def test_tables_equal_the_hits(eng, indir, query_dir, tmp_path):      # noqa: F811
    from pyani_amd.subcmd_search import run_screen_search, search_tab_path
    eng.clear_genomes()
    run = run_screen_search(indir, query_dir, tmp_path, min_identity=0.8, scale=16, write_output=True, engine=eng)
    assert eng.genome_count() == 0 and run.exact is None
    with pytest.raises(Exception):      # the run left no index behind
        eng.screen_search_count([])
    hits = run.hits
    assert hits.query_labels == list(QUERIES) and hits.db_labels == list(STEMS)
    assert [(hits.query_labels[a], hits.db_labels[b]) for a, b in hits.pairs()] == KEPT
    own = hits.a == hits.b      # the db's first three are the queries
    assert (hits.shared[own] == hits.query_sizes[hits.a[own]]).all() and (hits.identity()[own] == 1.0).all()
    assert (hits.identity()[~own] > 0.9).all() and (hits.identity()[~own] < 1.0).all()
    assert run.written == [search_tab_path(tmp_path, "hits"), search_tab_path(tmp_path, "best")]
    assert list(run.frame.columns) == ["query", "db", "shared", "containment_query", "containment_db", "identity"]
    _same_table(_read(run.written[0]), hits.frame())
    _same_table(_read(run.written[1]), hits.best(1).frame())
    assert [(q, d) for q, d in zip(run.best.frame()["query"], run.best.frame()["db"])] == [(q, q) for q in QUERIES]
    two = run_screen_search(indir, query_dir, min_identity=0.8, scale=16, top=2, engine=eng)
    assert len(two.best.a) == 6 and two.written == [] and (two.hits.shared == hits.shared).all()


def test_exact_anim_equals_plain_anim_pairs(eng, indir, query_dir, tmp_path):      # noqa: F811
    from pyani_amd import anim, files
    from pyani_amd.subcmd_search import run_screen_search, search_tab_path
    eng.clear_genomes()
    run = run_screen_search(indir, query_dir, tmp_path, min_identity=0.8, scale=16, exact="anim", write_output=True, engine=eng)
    assert eng.genome_count() == 0
    assert [(run.hits.query_labels[a], run.hits.db_labels[b]) for a, b in run.hits.pairs()] == KEPT
    assert sorted(run.exact) == sorted(set(KEPT) | {(d, q) for q, d in KEPT})      # both directions of every kept pair
    paths = files.get_fasta_paths(indir)
    ids = {p.stem: gid for p, (gid, _, _) in zip(paths, eng.add_fasta_batch(paths))}
    try:
        keys = sorted(run.exact)
        recs = eng.anim_pairs([ids[r] for r, _ in keys], [ids[q] for _, q in keys])
        for key, rec in zip(keys, recs):
            assert run.exact[key] == anim._tuple(rec), key
    finally:
        eng.clear_genomes()
    f = run.frame
    assert list(f.columns)[6:] == ["anim_identity_query", "anim_coverage_query", "anim_identity_db", "anim_coverage_db"]
    for row in f.itertuples():
        fwd, rev = run.exact[(row.query, row.db)], run.exact[(row.db, row.query)]
        assert row.anim_identity_query == fwd[2] and row.anim_identity_db == rev[2]
        assert row.anim_coverage_query == fwd[0] / run.query_lengths[row.query] and row.anim_coverage_db == rev[0] / run.db_lengths[row.db]
        assert 0.9 < row.anim_identity_query <= 1.0 and 0.9 < row.anim_coverage_query <= 1.0
    _same_table(_read(search_tab_path(tmp_path, "hits")), f)
