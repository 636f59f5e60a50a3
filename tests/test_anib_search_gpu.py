"""The ANIb search mode on the GPU (pg_anib_set_search, Engine.anib_set_search): with "all_diagonals" the fragment kernel's preliminary
stage also walks the diagonals of a candidate's band that hold no seed.  The bar is EQUALITY, row for row and field for field, with
the host statement of the same mode (oracle/anib_cpu.cpp with ANIB_ALL_DIAGS set; tests/anib_search_cases.py sets and removes the
variable around each host call), and unchanged default-mode tables before, beside and after the mode.

The genomes are synth.genome(20250302, 6, g, 150_000): about 130 fragments per ordered pair."""
import json

import numpy as np
import pytest

from tests import anib_search_cases as cases

pytestmark = pytest.mark.gpu

ON, OFF = "all_diagonals", "seeds"


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    assert e.anib_search == OFF      # a fresh engine searches as it always has
    e.ids = [e.add_genome(*g) for g in cases.genomes()]
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _mode_is_off_between_tests(eng):
    yield
    assert eng.anib_search == OFF


class mode:
    """The engine in `name` mode inside the block, back in default mode after it."""
    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        self.eng.anib_set_search(self.name)
        assert self.eng.anib_search == self.name

    def __exit__(self, *exc):
        self.eng.anib_set_search(OFF)


def _assert_tuple(rec, want_rows, where):
    import anib_cpu
    aln, err, pid, kept = anib_cpu.reduce_rows(want_rows)
    assert (int(rec["aln_length"]), int(rec["sim_errors"]), int(rec["n_kept"])) == (aln, err, len(kept)), where
    assert abs(float(rec["pid"]) - pid) <= 1e-12 * max(1.0, pid) and int(rec["status"]) == 0, where


def _assert_pair_equals_host(eng, monkeypatch, q, s, qdata, sdata, fragsize=1020, want=None):
    """Engine in ON mode: anib_pair_rows == the host statement with the variable set, anib_pairs == reduce_rows of those rows."""
    if want is None:
        want = cases.host_pair(monkeypatch, qdata, sdata, ON, fragsize)
    with mode(eng, ON):
        got = eng.anib_pair_rows(q, s, fragsize)
        rec = eng.anib_pairs([q], [s], fragsize)[0]
    assert cases.rows_of(got) == cases.rows_of(want), (q, s, len(got), len(want))
    _assert_tuple(rec, want, (q, s))
    return want


# ---- 1. mode on: rows equal the host statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", cases.DIVERGED)
def test_mode_rows_and_tuple_equal_host_statement(eng, monkeypatch, pair):
    q, s = pair
    want = cases.host_rows(monkeypatch, q, s, ON)
    assert len(want) > 100
    _assert_pair_equals_host(eng, monkeypatch, eng.ids[q], eng.ids[s], None, None, want=want)


def test_mode_rows_batch_equals_host_statement(eng, monkeypatch):
    qs, ss = [eng.ids[q] for q, _ in cases.DIVERGED], [eng.ids[s] for _, s in cases.DIVERGED]
    with mode(eng, ON):
        res, off, rows = eng.anib_rows_batch(qs, ss)
    assert len(off) == len(qs) + 1 and int(off[0]) == 0 and int(off[-1]) == len(rows)
    for i, (q, s) in enumerate(cases.DIVERGED):
        want = cases.host_rows(monkeypatch, q, s, ON)
        assert cases.rows_of(rows[int(off[i]):int(off[i + 1])]) == cases.rows_of(want), (q, s)
        _assert_tuple(res[i], want, (q, s))


# ---- 2. both modes against the independent oracle ------------------------------------------------------------------------------
def test_mode_agrees_with_independent_oracle_at_least_as_often(eng, monkeypatch):
    total = {OFF: 0, ON: 0}
    host_total = used_total = 0
    for q, s in cases.ORACLE_PAIRS:
        same = {}
        for m in (OFF, ON):
            with mode(eng, m):
                used, same[m] = cases.oracle_agreement(eng.anib_pair_rows(eng.ids[q], eng.ids[s]), q, s)
            total[m] += same[m]
        print(f"pair ({q}, {s}): oracle uses {used} rows; identical: default {same[OFF]}, all diagonals {same[ON]}")
        assert same[ON] >= same[OFF], (q, s, same)
        used_total += used
        host_total += cases.oracle_agreement(cases.host_rows(monkeypatch, q, s, ON), q, s)[1]
    print(f"total: {used_total} used rows; identical: default {total[OFF]}, all diagonals {total[ON]}, host statement of the mode {host_total}")
    assert total[ON] == host_total > total[OFF]


# ---- 3. mode on: close pairs unchanged -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", cases.CLOSE)
def test_mode_leaves_close_pairs_as_they_are(eng, pair):
    q, s = (eng.ids[k] for k in pair)
    default = eng.anib_pair_rows(q, s)
    with mode(eng, ON):
        got = eng.anib_pair_rows(q, s)
    assert cases.rows_of(got) == cases.rows_of(default) and len(default) > 100


# ---- 4. default mode after the mode was on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", cases.DIVERGED)
def test_default_mode_after_the_mode_was_on(eng, monkeypatch, pair):
    q, s = pair
    with mode(eng, ON):
        eng.anib_pair_rows(eng.ids[q], eng.ids[s])
    assert eng.anib_search == OFF
    want = cases.host_rows(monkeypatch, q, s, OFF)
    assert cases.rows_of(eng.anib_pair_rows(eng.ids[q], eng.ids[s])) == cases.rows_of(want), pair
    _assert_tuple(eng.anib_pairs([eng.ids[q]], [eng.ids[s]])[0], want, pair)


def test_unknown_value_is_refused_and_the_setting_stays(eng):
    from pyani_amd import _lib
    with mode(eng, ON):
        assert eng.lib.pg_anib_set_search(eng._h, 2) == _lib.PG_E_ARG
        assert eng.anib_search == ON
        with pytest.raises(ValueError):
            eng.anib_set_search("bogus")
        assert eng.anib_search == ON
    from pyani_amd.engine import Engine
    with Engine(0) as fresh:
        assert fresh.anib_search == OFF


# ---- 5. edge inputs, mode on ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(eng):
    """25 kb relatives of genomes 4 and 5 plus the degenerate genomes: {name: (engine id, data)}."""
    from pyani_amd import synth
    data = {
        "g4": synth.genome(cases.SEED, cases.N, 4, 25_000),
        "g5": synth.genome(cases.SEED, cases.N, 5, 25_000),
        "tiny": (np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8), np.array([0, 14], dtype=np.uint64)),
        "alln": (np.frombuffer(b"N" * 3000, dtype=np.uint8), np.array([0, 3000], dtype=np.uint64)),
        "empty": (np.zeros(0, dtype=np.uint8), np.array([0, 0], dtype=np.uint64)),
    }
    return {k: (eng.add_genome(*v), v) for k, v in data.items()}


@pytest.mark.parametrize("q,s,fragsize", [("g4", "g4", 1020), ("g5", "tiny", 1020), ("tiny", "g5", 1020), ("g5", "alln", 1020),
                                          ("alln", "g5", 1020), ("g5", "empty", 1020), ("empty", "g5", 1020), ("g5", "g4", 500),
                                          ("g4", "g5", 500)])
def test_edge_inputs_in_the_mode_equal_host_statement(eng, monkeypatch, small, q, s, fragsize):
    want = _assert_pair_equals_host(eng, monkeypatch, small[q][0], small[s][0], small[q][1], small[s][1], fragsize)
    if q == s:
        assert len(want) >= 24
    elif {q, s} == {"g4", "g5"}:
        assert len(want) > 30
    else:
        assert len(want) == 0


# ---- 6. windows off the subject's ends and across a record boundary ----------------------------------------------------------------
def test_bands_that_leave_the_subject_or_cross_a_record_boundary(eng, monkeypatch):
    # The query's fragments are diverged copies of the subject's first 3 kb, its last 3 kb and the 3 kb around the boundary of its two
    # records, in both orientations.  A candidate's diagonal there is within a few bases of 0, of (subject length - fragment end) or of
    # the boundary, so the +-47 diagonals the mode walks reach BEFORE base 0 of the subject's arrays, PAST their last base and INTO
    # THE OTHER RECORD: the 32-base windows of those walks lie partly or wholly outside what may be read or matched.
    query, subject = cases.ends_case()
    q, s = eng.add_genome(*query), eng.add_genome(*subject)
    want = _assert_pair_equals_host(eng, monkeypatch, q, s, query, subject)
    rows = cases.rows_of(want)
    starts = {(r[10], min(r[8], r[9])) for r in rows}
    ends = {(r[10], max(r[8], r[9])) for r in rows}
    assert (0, 1) in starts or (1, 1) in starts          # an alignment that begins at the first base of a record
    assert (0, 20_000) in ends or (1, 20_000) in ends    # ... and one that ends at the last
    assert {r[10] for r in rows} == {0, 1} and len(rows) >= 16


# ---- 7. overlapping neighbourhoods ---------------------------------------------------------------------------------------------
def test_second_candidate_band_is_cut_by_the_first_ones_neighbourhood(eng, monkeypatch):
    # cases.TANDEM_UNIT = 90 (not 70: at 70 the final alignment bridges the duplication and the fragment has one row; see there)
    query, subject = cases.tandem_case()
    q, s = eng.add_genome(*query), eng.add_genome(*subject)
    want = _assert_pair_equals_host(eng, monkeypatch, q, s, query, subject)
    frags = [int(r["frag"]) for r in want]
    assert max(frags.count(f) for f in set(frags)) >= 2      # two candidates of one fragment, cases.TANDEM_UNIT diagonals apart
    assert 48 <= cases.TANDEM_UNIT < 95


# ---- 8. driver -----------------------------------------------------------------------------------------------------------------
def test_run_anib_in_the_mode_writes_the_modes_tables_and_its_record(eng, tmp_path):
    from pyani_amd import anib, anim, subcmd_anib as sa, synth
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir()
    stems = ["syn00004", "syn00005"]
    for g, stem in zip((4, 5), stems):
        synth.write_fasta(indir / f"{stem}.fna", *synth.genome(cases.SEED, cases.N, g, 60_000), stem)
    first = eng.genome_count()
    run = sa.run_anib(indir, outdir, write_output=True, engine=eng, search=ON)
    assert eng.anib_search == OFF      # the engine's own setting is back
    assert json.loads((outdir / sa.RUN_RECORD).read_text())["search"] == ON and sa.recorded_search(outdir) == ON
    ids = dict(zip(stems, (first, first + 1)))      # sorted stems, added in that order
    differs = 0
    for qs, ss in ((stems[0], stems[1]), (stems[1], stems[0])):
        with mode(eng, ON):
            rows = eng.anib_pair_rows(ids[qs], ids[ss])
            rec = eng.anib_pairs([ids[qs]], [ids[ss]])[0]
        differs += cases.rows_of(rows) != cases.rows_of(eng.anib_pair_rows(ids[qs], ids[ss]))
        recs = anim.fasta_records(indir / f"{ss}.fna")
        want = tmp_path / f"want_{qs}_{ss}.tab"
        assert anib.write_blast_tab(want, rows, [r[0] for r in recs], [r[1] for r in recs]) > 40
        assert sa.table_path(outdir, qs, ss).read_text() == want.read_text()
        assert run.results[(qs, ss)] == (int(rec["aln_length"]), int(rec["sim_errors"]), float(rec["pid"]))
    print(f"pairs whose table differs between the modes: {differs} of 2")
    with pytest.raises(ValueError):
        sa.run_anib(indir, outdir, recovery=True, engine=eng, search=OFF)
    again = sa.run_anib(indir, outdir, recovery=True, engine=eng, search=ON)      # the same mode recovers
    assert len(again.recovered) == 2 and again.results == run.results


# ---- 9. multi-engine -----------------------------------------------------------------------------------------------------------
def test_multi_engine_sets_every_engine(eng):
    from pyani_amd.multi import MultiEngine
    pairs = [(5, 4), (4, 5)]      # the mode changes rows of both
    default = eng.anib_pairs([eng.ids[a] for a, _ in pairs], [eng.ids[b] for _, b in pairs])
    with mode(eng, ON):
        want = eng.anib_pairs([eng.ids[a] for a, _ in pairs], [eng.ids[b] for _, b in pairs])
    assert [tuple(r) for r in want] != [tuple(r) for r in default]
    with MultiEngine([0]) as multi:
        assert multi.anib_search == OFF
        ids = {k: multi.add_genome(*cases.genomes()[k]) for k in (4, 5)}
        multi.anib_set_search(ON)
        assert all(e.anib_search == ON for e in multi.engines) and multi.anib_search == ON
        got = multi.anib_pairs([ids[a] for a, _ in pairs], [ids[b] for _, b in pairs])
        with pytest.raises(ValueError):
            multi.anib_set_search("bogus")
        assert multi.anib_search == ON
    assert [tuple(r) for r in got] == [tuple(r) for r in want]
