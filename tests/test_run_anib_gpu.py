"""run_anib (pyani_amd/subcmd_anib.py): the legacy ANIb run — fragment files, one .blast_tab per ordered pair under blastn_output/,
recovery (--skip_blastn), the five matrices — on three synthetic genomes."""
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, str(ROOT / "oracle"))

pytestmark = pytest.mark.gpu

STEMS = ("syn.v1.0", "synB", "synC")      # (a stem with dots)


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def indir(tmp_path_factory):
    from pyani_amd import synth
    d = tmp_path_factory.mktemp("anib_in")
    for k, stem in enumerate(STEMS):
        seq, _ = synth.genome(20250302, 6, k, 30_000)
        off = np.array([0, len(seq) // 3, len(seq)] if k == 1 else [0, len(seq)], dtype=np.uint64)      # synB: two records
        synth.write_fasta(d / f"{stem}.fna", seq, off, stem)
    return d


def _same_results(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k][:2] == b[k][:2] and abs(a[k][2] - b[k][2]) <= 1e-12 * max(1.0, abs(b[k][2])), (k, a[k], b[k])


def _same_matrices(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        x, y = a[name], b[name]
        assert list(x.index) == list(y.index) and list(x.columns) == list(y.columns)
        np.testing.assert_allclose(x.values, y.values, rtol=1e-12, atol=0.0, equal_nan=True, err_msg=name)


def test_run_writes_the_legacy_files_and_recovers_from_them(eng, indir, tmp_path):
    import anib_oracle
    from pyani_amd import _lib, anib, anim
    from pyani_amd.subcmd_anib import run_anib
    out = tmp_path / "out"
    eng.clear_genomes()
    run = run_anib(indir, out, write_output=True, engine=eng)
    pairs = [(q, s) for q in STEMS for s in STEMS if q != s]
    bdir = out / "blastn_output"
    assert sorted(p.name for p in bdir.iterdir()) == sorted([f"{q}_vs_{s}.blast_tab" for q, s in pairs] + [f"{s}-fragments.fna" for s in STEMS])
    assert run.written == [bdir / f"{q}_vs_{s}.blast_tab" for q, s in pairs] and run.recovered == [] and eng.genome_count() == 0
    assert list(run.results) == pairs and sorted(run.fraglengths) == sorted(STEMS)
    assert run.fraglengths["synB"] == anib.get_fragment_lengths(bdir / "synB-fragments.fna") and len(run.fraglengths["synB"]) >= 30
    # every table is what write_blast_tab makes of that pair's anib_pair_rows, and parses back to the run's tuple
    ids = {s: eng.add_fasta(indir / f"{s}.fna")[0] for s in STEMS}
    for q, s in pairs:
        recs = anim.fasta_records(indir / f"{s}.fna")
        ref = tmp_path / "ref.blast_tab"
        n = anib.write_blast_tab(ref, eng.anib_pair_rows(ids[q], ids[s]), [r[0] for r in recs], [r[1] for r in recs])
        assert n > 20 and (bdir / f"{q}_vs_{s}.blast_tab").read_bytes() == ref.read_bytes(), (q, s)
        for parse in (anib.parse_blast_tab, anib_oracle.parse_blast_tab):
            kw = {"engine": eng} if parse is anib.parse_blast_tab else {}
            aln, err, pid = parse(bdir / f"{q}_vs_{s}.blast_tab", **kw)
            want = run.results[(q, s)]
            assert (aln, err) == want[:2] and abs(pid - want[2]) <= 1e-12 * max(1.0, want[2]), (q, s, parse.__module__)
    eng.clear_genomes()
    res, lengths = anib.calculate_anib_pairs(sorted(indir.glob("*.fna")), engine=eng)
    assert run.lengths == lengths and {k: run.results[k] for k in res} == res
    _same_matrices(run.matrices, anib.process_blast_results(res, lengths))
    # without write_output: the same tuples from one anib_pairs call, nothing written
    plain = run_anib(indir, engine=eng)
    assert plain.results == run.results and plain.written == [] and plain.fraglengths is None
    # recovery: two tables gone
    gone = [bdir / f"{q}_vs_{s}.blast_tab" for q, s in (pairs[1], pairs[4])]
    kept = [f for f in run.written if f not in gone]
    before = {f: (f.stat().st_mtime_ns, f.read_bytes()) for f in kept}
    for f in gone:
        f.unlink()
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        again = run_anib(indir, out, recovery=True, write_output=True, engine=eng)
        assert again.recovered == kept and again.written == gone
        assert {f: (f.stat().st_mtime_ns, f.read_bytes()) for f in kept} == before
        assert eng.profile_get(_lib.K_ANIB_FRAG)[1] > 0 and eng.profile_get(_lib.K_ANIB_ROWS_PACK)[1] > 0
        _same_results(again.results, run.results)
        _same_matrices(again.matrices, run.matrices)
        # all six present: nothing is searched
        eng.profile_reset()
        third = run_anib(indir, out, recovery=True, write_output=True, engine=eng)
        assert len(third.recovered) == 6 and third.written == []
        assert eng.profile_get(_lib.K_ANIB_FRAG)[1] == 0 and eng.profile_get(_lib.K_ANIB_BUCKET)[1] == 0
        _same_results(third.results, run.results)
        _same_matrices(third.matrices, run.matrices)
    finally:
        eng.profile_enable(False)


def test_output_directory_is_required_before_any_work(eng, indir):
    from pyani_amd.subcmd_anib import run_anib
    eng.clear_genomes()
    for kw in (dict(write_output=True), dict(recovery=True)):
        with pytest.raises(ValueError):
            run_anib(indir, None, engine=eng, **kw)
    assert eng.genome_count() == 0


def test_duplicate_stem_raises(eng, indir, tmp_path):
    import shutil
    from pyani_amd.subcmd_anib import run_anib
    d = tmp_path / "dup"
    d.mkdir()
    shutil.copy(indir / "synB.fna", d / "synB.fna")
    shutil.copy(indir / "synC.fna", d / "synB.fa")
    with pytest.raises(ValueError):
        run_anib(d, engine=eng)
