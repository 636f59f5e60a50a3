"""Screened runs: run_anim / run_anib with screen=... (pyani_amd/subcmd_anim.py, pyani_amd/subcmd_anib.py) on six synthetic genomes —
two families of three at about 95 % identity, unrelated across families (tests/screen_select_cases.run_genomes).  The kept pairs must
come out exactly as the unscreened run gives them, the dropped ones must be absent everywhere and NaN in the matrices."""
import json

import numpy as np
import pandas as pd
import pytest

from tests import screen_select_cases as ssc

pytestmark = pytest.mark.gpu

STEMS = ssc.RUN_STEMS
ALL = [(q, s) for q in STEMS for s in STEMS if q != s]
KEPT = ssc.RUN_KEPT
DROPPED = [p for p in ALL if p not in KEPT]


def _options():
    from pyani_amd.screen import ScreenOptions
    return ScreenOptions(0.8, scale=16)


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def indir(tmp_path_factory):
    from pyani_amd import synth
    d = tmp_path_factory.mktemp("screened_in")
    for stem, (seq, off) in zip(STEMS, ssc.run_genomes()):
        synth.write_fasta(d / f"{stem}.fna", seq, off, stem)
    return d


@pytest.fixture(scope="module")
def anim_runs(eng, indir, tmp_path_factory):
    """(unscreened run, its directory, screened run, its directory): computed once, shared, not written to."""
    from pyani_amd.subcmd_anim import run_anim
    plain_dir, scr_dir = tmp_path_factory.mktemp("anim_plain"), tmp_path_factory.mktemp("anim_screened")
    eng.clear_genomes()
    plain = run_anim(indir, plain_dir, skip_zero=True, write_output=True, engine=eng)
    screened = run_anim(indir, scr_dir, skip_zero=True, write_output=True, engine=eng, screen=_options())
    return plain, plain_dir, screened, scr_dir


@pytest.fixture(scope="module")
def anib_runs(eng, indir, tmp_path_factory):
    from pyani_amd.subcmd_anib import run_anib
    plain_dir, scr_dir = tmp_path_factory.mktemp("anib_plain"), tmp_path_factory.mktemp("anib_screened")
    eng.clear_genomes()
    plain = run_anib(indir, plain_dir, write_output=True, engine=eng)
    screened = run_anib(indir, scr_dir, write_output=True, engine=eng, screen=_options())
    return plain, plain_dir, screened, scr_dir


def _design(screened):
    """The design of the input, asserted first: the screen keeps exactly the 12 within-family ordered pairs and drops the other 18."""
    assert len(KEPT) == 12 and len(DROPPED) == 18
    assert screened is not None and screened.labels == list(STEMS) and screened.options == _options()
    assert [(STEMS[a], STEMS[b]) for a, b in screened.pairs()] == KEPT
    assert screened.sizes.min() > 3000 and screened.identity().min() > 0.9 and screened.shared.min() > 1000


def _pairs_tab(outdir, screened):
    tab = pd.read_csv(outdir / "screen_output" / "screen_pairs.tab", sep="\t", float_precision="round_trip")
    assert list(tab.columns) == ["query", "subject", "shared", "containment", "identity"]
    assert list(zip(tab["query"], tab["subject"])) == KEPT and (tab["shared"].to_numpy() == screened.shared).all()
    assert (tab["identity"].to_numpy() == screened.identity()).all() and (tab["containment"].to_numpy() == screened.containment()).all()


def _cells(frame, rows, cols, pairs):
    r, c = list(frame.index), list(frame.columns)
    v = frame.to_numpy(dtype=np.float64)
    return np.array([v[r.index(rows[q]), c.index(cols[s])] for q, s in pairs])


def test_screened_run_anim(anim_runs):
    plain, plain_dir, run, scr_dir = anim_runs
    _design(run.screened)
    assert plain.screened is None and len(plain) == len(run) == 9
    assert set(KEPT) <= set(plain.results)      # the unscreened run aligned every within-family pair
    assert sorted(run.results) == sorted(KEPT) and all(run.results[p] == plain.results[p] for p in KEPT)
    assert list(run.results) == [p for p in plain.results if p in KEPT]      # the run's own order (the subject varies slowest), less the dropped
    gid = run.genome_ids
    assert gid == plain.genome_ids and run.lengths == plain.lengths
    key = lambda row: (row["query_id"], row["subject_id"])
    assert {key(r): r for r in run.comparisons} == {key(r): r for r in plain.comparisons if (r["query_id"], r["subject_id"]) in {(gid[q], gid[s]) for q, s in KEPT}}
    assert len(run.comparisons) == 12
    assert sorted(run.matrices) == sorted(plain.matrices) and len(run.matrices) == 5
    for name, frame in run.matrices.items():
        assert np.array_equal(_cells(frame, gid, gid, KEPT), _cells(plain.matrices[name], gid, gid, KEPT)), name
        assert not np.isnan(_cells(frame, gid, gid, KEPT)).any() and np.isnan(_cells(frame, gid, gid, DROPPED)).all(), name
        assert np.array_equal(np.diag(frame.to_numpy()), np.diag(plain.matrices[name].to_numpy())), name
    # files: only the kept pairs, byte for byte the unscreened run's
    from pyani_amd.subcmd_anim import outfile_path
    found = sorted(p for p in (scr_dir / "nucmer_output").glob("*/*") if p.is_file())
    assert found == sorted(outfile_path(scr_dir, q, s) for q, s in KEPT) and sorted(run.written) == found and run.recovered == []
    for q, s in KEPT:
        assert outfile_path(scr_dir, q, s).read_bytes() == outfile_path(plain_dir, q, s).read_bytes(), (q, s)
    assert len(plain.written) == 30
    _pairs_tab(scr_dir, run.screened)


def test_screened_run_anib(anib_runs):
    plain, plain_dir, run, scr_dir = anib_runs
    _design(run.screened)
    assert plain.screened is None and len(plain) == len(run) == 7
    assert list(plain.results) == ALL and list(run.results) == KEPT and all(run.results[p] == plain.results[p] for p in KEPT)
    assert run.lengths == plain.lengths
    same = {s: s for s in STEMS}
    for name, frame in run.matrices.items():
        assert list(frame.index) == list(frame.columns) == list(STEMS)
        assert np.array_equal(_cells(frame, same, same, KEPT), _cells(plain.matrices[name], same, same, KEPT)), name
        assert not np.isnan(_cells(frame, same, same, KEPT)).any(), name
        assert np.isnan(_cells(frame, same, same, DROPPED)).all(), (name, _cells(frame, same, same, DROPPED))      # NaN, not a perfect match
        assert not np.isnan(_cells(plain.matrices[name], same, same, DROPPED)).any(), name
        assert np.array_equal(np.diag(frame.to_numpy()), np.diag(plain.matrices[name].to_numpy())), name
    from pyani_amd.subcmd_anib import table_path
    tables = sorted((scr_dir / "blastn_output").glob("*.blast_tab"))
    assert tables == sorted(table_path(scr_dir, q, s) for q, s in KEPT) and run.written == [table_path(scr_dir, q, s) for q, s in KEPT]
    for q, s in KEPT:
        assert table_path(scr_dir, q, s).read_bytes() == table_path(plain_dir, q, s).read_bytes(), (q, s)
    assert len(plain.written) == 30 and len(list((scr_dir / "blastn_output").glob("*-fragments.fna"))) == 6
    _pairs_tab(scr_dir, run.screened)
    record = json.loads((scr_dir / "anib_run.json").read_text())
    assert record == {"search": "seeds", "fragsize": 1020, "screen": {"min_identity": 0.8, "kmer": 16, "scale": 16, "min_shared": 2}}
    assert json.loads((plain_dir / "anib_run.json").read_text()) == {"search": "seeds", "fragsize": 1020}


def _frames_equal(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert list(a[name].index) == list(b[name].index) and list(a[name].columns) == list(b[name].columns)
        assert np.array_equal(a[name].to_numpy(dtype=np.float64), b[name].to_numpy(dtype=np.float64), equal_nan=True), name


def test_a_threshold_of_zero_is_the_unscreened_run(eng, indir, anim_runs, anib_runs):
    from pyani_amd.subcmd_anib import run_anib
    from pyani_amd.subcmd_anim import run_anim
    eng.clear_genomes()
    plain = anim_runs[0]
    run = run_anim(indir, skip_zero=True, engine=eng, screen=0.0)
    assert len(run.screened.a) == 30 and run.results == plain.results and list(run.results) == list(plain.results)
    _frames_equal(run.matrices, plain.matrices)
    assert run.json == plain.json and run.comparisons == plain.comparisons
    plain = anib_runs[0]
    run = run_anib(indir, engine=eng, screen=0.0)
    assert len(run.screened.a) == 30 and run.results == plain.results and list(run.results) == ALL
    _frames_equal(run.matrices, plain.matrices)


def test_recovery_of_a_screened_directory_recomputes_nothing(eng, indir, anim_runs, anib_runs):
    from pyani_amd import _lib
    from pyani_amd.screen import ScreenOptions
    from pyani_amd.subcmd_anib import run_anib
    from pyani_amd.subcmd_anim import run_anim
    eng.clear_genomes()
    eng.profile_enable(True)
    try:
        _, _, first, scr_dir = anim_runs
        eng.profile_reset()
        again = run_anim(indir, scr_dir, recovery=True, skip_zero=True, write_output=True, engine=eng, screen=_options())
        assert sorted(again.recovered) == sorted(first.written) and again.written == []
        assert eng.profile_get(_lib.K_ANIM_SEED)[1] == 0 and eng.profile_get(_lib.K_ANIM_EXTEND)[1] == 0
        assert again.results == first.results and [(STEMS[a], STEMS[b]) for a, b in again.screened.pairs()] == KEPT
        _frames_equal(again.matrices, first.matrices)
        _, _, first, scr_dir = anib_runs
        eng.profile_reset()
        again = run_anib(indir, scr_dir, recovery=True, write_output=True, engine=eng, screen=_options())
        assert again.recovered == first.written and again.written == []
        assert eng.profile_get(_lib.K_ANIB_FRAG)[1] == 0 and eng.profile_get(_lib.K_ANIB_BUCKET)[1] == 0
        assert list(again.results) == KEPT
        for p in KEPT:
            assert again.results[p][:2] == first.results[p][:2] and abs(again.results[p][2] - first.results[p][2]) <= 1e-12 * first.results[p][2]
        for name in first.matrices:
            np.testing.assert_allclose(again.matrices[name].to_numpy(), first.matrices[name].to_numpy(), rtol=1e-12, atol=0.0, equal_nan=True, err_msg=name)
        # other options than the directory's record, none included, and a screen over an unscreened directory: refused before any work
        for other in (ScreenOptions(0.9, scale=16), ScreenOptions(0.8), 0.8, None):
            with pytest.raises(ValueError, match="recovery"):
                run_anib(indir, scr_dir, recovery=True, engine=eng, screen=other)
        with pytest.raises(ValueError, match="recovery"):
            run_anib(indir, anib_runs[1], recovery=True, engine=eng, screen=_options())
        assert eng.profile_get(_lib.K_ANIB_FRAG)[1] == 0 and eng.genome_count() == 0
    finally:
        eng.profile_enable(False)


def test_a_collective_run_refuses_a_screen(eng, indir):
    from pyani_amd.subcmd_anim import run_anim
    eng.clear_genomes()
    for kw in (dict(distributed=True), dict(group=object())):
        with pytest.raises(ValueError, match="collective"):
            run_anim(indir, engine=eng, screen=_options(), **kw)
    assert eng.genome_count() == 0
