"""GPU: run_anim_components (pyani_amd/subcmd_components.py) on the six genomes of the screened runs — two families of three
(tests/screen_select_cases.run_genomes): ANIm over the kept pairs only, assembled per connected component.  Everything must equal the
screened run_anim over the same directory: the results, and each component's frames as the sub-blocks of the run's frames."""
import numpy as np
import pandas as pd
import pytest

from tests.test_run_screened_gpu import KEPT, STEMS, _options, anim_runs, eng, indir      # noqa: F401 — the fixtures of the screened runs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comp_run(eng, indir, tmp_path_factory):      # noqa: F811
    from pyani_amd.subcmd_components import run_anim_components
    out = tmp_path_factory.mktemp("anim_components")
    eng.clear_genomes()
    return run_anim_components(indir, out, screen=_options(), skip_zero=True, write_output=True, engine=eng), out


def test_components_of_the_two_families(comp_run):
    run, _ = comp_run
    sc = run.components
    assert [[STEMS[v] for v in sc.members(c).tolist()] for c in range(len(sc.size))] == [list(STEMS[:3]), list(STEMS[3:])]
    assert sc.size.tolist() == [3, 3] and sc.complete.tolist() == [True, True] and sc.edges.tolist() == [6, 6]      # no singletons
    assert sorted(run.runs) == [0, 1] and [run.runs[c].members for c in (0, 1)] == [list(STEMS[:3]), list(STEMS[3:])]
    assert [(STEMS[a], STEMS[b]) for a, b in run.screened.pairs()] == KEPT
    assert all(run.runs[c].representative == STEMS[int(sc.representative[c])] and run.runs[c].representative in run.runs[c].members for c in (0, 1))
    # the representative: the member that shares most with the others of its component
    for c in (0, 1):
        w = {s: int(run.screened.shared[run.screened.a == STEMS.index(s)].sum()) for s in run.runs[c].members}
        assert run.runs[c].representative == max(sorted(w), key=lambda s: w[s])


def test_results_equal_the_screened_run(comp_run, anim_runs):      # noqa: F811
    run, _ = comp_run
    _, _, screened, _ = anim_runs
    merged = {k: v for c in run.runs.values() for k, v in c.results.items()}
    assert sorted(merged) == sorted(KEPT) and merged == screened.results
    assert run.genome_ids == screened.genome_ids and run.lengths == screened.lengths
    key = lambda row: (row["query_id"], row["subject_id"])      # noqa: E731
    rows = {key(r): r for c in run.runs.values() for r in c.comparisons}
    assert rows == {key(r): r for r in screened.comparisons} and len(rows) == 12
    for c, fam in ((0, STEMS[:3]), (1, STEMS[3:])):
        sub = run.runs[c]
        gids = [screened.genome_ids[s] for s in fam]
        assert sub.genome_ids == {s: screened.genome_ids[s] for s in fam} and sub.lengths == {s: screened.lengths[s] for s in fam}
        assert sorted(sub.matrices) == sorted(screened.matrices) and len(sub.matrices) == 5
        for name, frame in sub.matrices.items():
            assert list(frame.index) == gids and list(frame.columns) == gids
            block = screened.matrices[name].loc[gids, gids].to_numpy(dtype=np.float64)
            got = frame.to_numpy(dtype=np.float64)
            assert got.shape == (3, 3) and np.array_equal(got, block) and not np.isnan(got).any(), (c, name)      # a complete component: no NaN
        assert sorted(sub.json) == sorted(screened.json)
        assert sub.json["df_identity"] == screened.matrices["identity"].loc[gids, gids].to_json()


def test_tables_round_trip(comp_run):
    run, out = comp_run
    d = out / "screen_output"
    assert sorted(p.name for p in d.iterdir()) == ["screen_components.tab", "screen_membership.tab", "screen_pairs.tab"]
    assert sorted(run.written) == sorted(d.iterdir()) and not (out / "nucmer_output").exists()      # no alignment files
    pairs = pd.read_csv(d / "screen_pairs.tab", sep="\t", float_precision="round_trip")
    assert list(zip(pairs["query"], pairs["subject"])) == KEPT and (pairs["shared"].to_numpy() == run.screened.shared).all()
    comp = pd.read_csv(d / "screen_components.tab", sep="\t")
    assert list(comp.columns) == ["component", "size", "representative", "edges", "complete"]
    want = run.components.frame()
    assert all((comp[c].to_numpy() == want[c].to_numpy()).all() for c in comp.columns)
    mem = pd.read_csv(d / "screen_membership.tab", sep="\t")
    assert list(mem.columns) == ["genome", "component", "representative"]
    assert mem["genome"].tolist() == list(STEMS) and mem["component"].tolist() == [0, 0, 0, 1, 1, 1]
    assert mem["representative"].tolist() == [run.runs[c].representative for c in (0, 0, 0, 1, 1, 1)]


def test_refuses_before_any_work(indir):      # noqa: F811
    from pyani_amd.subcmd_components import run_anim_components
    with pytest.raises(ValueError, match="screen"):
        run_anim_components(indir)
    with pytest.raises(ValueError, match="output directory"):
        run_anim_components(indir, screen=0.8, write_output=True)
