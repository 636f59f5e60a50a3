"""The fragment-mode (ANIb) kernels on the directed fragments of tests/anib_frag_cases.py: anib_bucket_kernel and anib_frag_kernel
(pga_frag.inc) restate by hand, for a wave, what pg_anib_core.h states for one thread — the X-drop band in registers with its lane
shuffles, the re-centring through LDS, the shared best score, the 32-base match windows, the rank-select of the seed list, the word
tier, the caps and the e-value cut in double precision — and every case goes where one of these can go wrong
(tests/test_anib_frag_cases_cpu.py shows that without a GPU).  The bar is EQUALITY with the host statement (oracle/anib_cpu.cpp), row for
row, all 12 fields, in order, for every case and without conditions."""
import json
import random

import pytest

from tests import anib_frag_cases as cases

pytestmark = pytest.mark.gpu

ON, OFF = "all_diagonals", "seeds"


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    assert e.anib_search == OFF
    ids = {}
    e.case_ids = {}
    for c in cases.all_cases():      # every genome once (cases of a group share their subject)
        for g in (c.query, c.subject):
            if id(g) not in ids:
                ids[id(g)] = e.add_genome(*g)
        e.case_ids[c.name] = (ids[id(c.query)], ids[id(c.subject)])
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _default_search_between_tests(eng):
    yield
    assert eng.anib_search == OFF


def _n_frags(case):
    off = case.query[1]
    return sum(-(-int(b - a) // case.fragsize) for a, b in zip(off[:-1], off[1:]))


def _assert_tuple(rec, want_rows, case):
    import anib_cpu
    want = [dict(zip(cases.FIELDS, r)) for r in want_rows]
    aln, err, pid, kept = anib_cpu.reduce_rows(want)
    got = (int(rec["aln_length"]), int(rec["sim_errors"]), int(rec["n_frags"]), int(rec["n_kept"]), int(rec["status"]))
    assert got == (aln, err, _n_frags(case), len(kept), 0), case.name
    assert abs(float(rec["pid"]) - pid) <= 1e-12 * max(1.0, pid), case.name      # (a mean of 3-decimal values: the order of the sum)


def _check_group(eng, monkeypatch, group, mode):
    eng.anib_set_search(mode)
    try:
        got = [(c, eng.anib_pair_rows(*eng.case_ids[c.name], c.fragsize), eng.anib_pairs(*([i] for i in eng.case_ids[c.name]), c.fragsize)[0])
               for c in cases.by_group(group)]
    finally:
        eng.anib_set_search(OFF)
    for c, rows, rec in got:
        want = cases.host_trace(c).rows if mode == OFF else cases.host_pair(monkeypatch, c, mode)
        assert cases.rows_of(rows) == want, (c.name, mode, len(rows), len(want))
        _assert_tuple(rec, want, c)


@pytest.mark.parametrize("group", cases.GROUPS)
def test_pair_rows_and_tuple_equal_host_statement(eng, monkeypatch, group):
    _check_group(eng, monkeypatch, group, OFF)


@pytest.mark.parametrize("group", cases.GROUPS)
def test_pair_rows_and_tuple_equal_host_statement_all_diagonals(eng, monkeypatch, group):
    _check_group(eng, monkeypatch, group, ON)
    if group == cases.GROUPS[-1]:      # back in the default search: the first group still has its default rows
        assert eng.anib_search == OFF
        _check_group(eng, monkeypatch, cases.GROUPS[0], OFF)


@pytest.mark.parametrize("fragsize", sorted({c.fragsize for c in cases.all_cases()}))
def test_one_batch_over_all_cases_of_a_fragment_size(eng, fragsize):
    batch = [c for c in cases.all_cases() if c.fragsize == fragsize]
    random.Random(fragsize).shuffle(batch)
    batch.append(batch[len(batch) // 2])      # one case twice
    res, off, rows = eng.anib_rows_batch([eng.case_ids[c.name][0] for c in batch], [eng.case_ids[c.name][1] for c in batch], fragsize)
    assert len(off) == len(batch) + 1 and int(off[0]) == 0 and int(off[-1]) == len(rows)
    assert cases.rows_of(eng.anib_rows_read(len(rows))) == cases.rows_of(rows)
    for i, c in enumerate(batch):
        want = cases.host_trace(c).rows
        assert cases.rows_of(rows[int(off[i]):int(off[i + 1])]) == want, (c.name, i)
        _assert_tuple(res[i], want, c)


def test_evalue_thresholds_equal_host_statement(eng):
    table = {}
    for c in cases.by_group("evalue"):
        dev, dev_mono = cases.lstar_of_rows(cases.rows_of(eng.anib_pair_rows(*eng.case_ids[c.name], c.fragsize)))
        host, host_mono = cases.lstar_of_rows(cases.host_trace(c).rows)
        assert dev_mono and host_mono, c.name
        table[c.name] = {"device": dev, "host": host}
        print(f"{c.name}: L* device {dev}, host {host}")
    print(json.dumps(table))      # (the values measured on an MI355X are kept in profiles/anib_frag_cases.json)
    assert len(table) == 24 and all(v["device"] == v["host"] is not None for v in table.values()), table
