"""GPU: pyani_amd.classify reproduces, for every golden case, exactly the sequence the reference's own code emitted
(tests/golden/classify, tools/make_classify_goldens.py): floats bit for bit, integers and booleans equal; memberships are the
stored networkx partitions, and the test-only restatement's (tests/classify_cases.py) where none are stored.  Both memory paths of
the sweep kernel (bit matrix in LDS up to 1024 genomes, in device memory beyond) are run and compared."""
import numpy as np
import pytest

from tests import classify_cases as cc
from tests.test_classify_cpu import assert_tuples, case_inputs, load_gold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


def as_tuples(seq):
    return [(s.interval, s.cliqueinfo.n_nodes, s.cliqueinfo.n_subgraphs, s.cliqueinfo.all_k_complete) for s in seq]


def partition_of(membership):
    groups = {}
    for node, rep in membership.items():
        groups.setdefault(rep, set()).add(node)
    assert all(rep in members for rep, members in groups.items())
    return {frozenset(v) for v in groups.values()}


def run_case(eng, name, gold, memberships):
    from pyani_amd import classify
    if "json" in gold:
        return classify.classify_run(gold["json"], gold["label_dict"], memberships=memberships, engine=eng, **gold["params"])
    I, C, labels = cc.build_case(name)
    return classify.classify(I, C, labels, memberships=memberships, engine=eng, **gold["params"])


@pytest.mark.parametrize("name", list(cc.CASES))
def test_golden_sequence_and_memberships(eng, name):
    gold = load_gold(name)
    if gold["raises"]:
        with pytest.raises(IndexError):
            run_case(eng, name, gold, "none")
        return
    seq = run_case(eng, name, gold, "all")
    assert_tuples(as_tuples(seq), gold["tuples"], name)
    labels = gold["labels"]
    if "partitions" in gold:
        want = [{frozenset(labels[g] for g in comp) for comp in step} for step in gold["partitions"]]
    else:
        I, C = case_inputs(name, gold)
        _, parts = cc.restate(I, C, partitions=True, **gold["params"])
        want = [{frozenset(labels[g] for g in comp) for comp in step} for step in parts]
    assert len(want) == len(seq)
    at = {lab: g for g, lab in enumerate(labels)}
    for k, (s, w) in enumerate(zip(seq, want)):
        assert len(s.membership) == s.cliqueinfo.n_nodes
        assert partition_of(s.membership) == w, f"{name}: membership of step {k} is not the expected partition"
        for node, rep in s.membership.items():      # the representative is the component's first member in label order
            assert at[rep] <= at[node]


@pytest.mark.parametrize("name", ["n12_default", "n60_coarse", "n200_default", "n12_json"])
def test_special_and_none_are_subsets_of_all(eng, name):
    gold = load_gold(name)
    full, special, none = (run_case(eng, name, gold, m) for m in ("all", "special", "none"))
    assert as_tuples(full) == as_tuples(special) == as_tuples(none)
    assert any(s.cliqueinfo.all_k_complete for s in full) and not all(s.cliqueinfo.all_k_complete for s in full)
    for f, s, o in zip(full, special, none):
        assert o.membership is None
        assert s.membership == (f.membership if f.cliqueinfo.all_k_complete else None)
    from pyani_amd.classify import special_intervals
    assert [s.interval for s in special_intervals(special)] == [t[0] for t in gold["tuples"] if t[3]]


def test_device_memory_path_equals_lds_path(eng, monkeypatch):
    """The 1500-genome case runs with the bit matrix in device memory; its leading 900 x 900 sub-matrix fits the LDS path too and is
    run through both (PYANI_CLASSIFY_GLOBAL, a development switch honoured under PYANI_DEV_KNOBS=1): same answers, and both equal
    the restatement."""
    from pyani_amd import classify
    I, C, labels = cc.build_case("n1500_default")
    I, C, labels = np.ascontiguousarray(I[:900, :900]), np.ascontiguousarray(C[:900, :900]), labels[:900]
    kw = dict(resolution=1e-3, memberships="all", engine=eng)
    monkeypatch.delenv("PYANI_CLASSIFY_GLOBAL", raising=False)
    lds = classify.classify(I, C, labels, **kw)
    monkeypatch.setenv("PYANI_CLASSIFY_GLOBAL", "1")
    glob = classify.classify(I, C, labels, **kw)
    monkeypatch.delenv("PYANI_CLASSIFY_GLOBAL")
    assert lds == glob
    want, parts = cc.restate(I, C, resolution=1e-3, partitions=True)
    assert_tuples(as_tuples(lds), want, "900 x 900 sub-matrix")
    for s, p in zip(lds, parts):
        assert partition_of(s.membership) == {frozenset(labels[g] for g in comp) for comp in p}


@pytest.mark.parametrize("n", [1024, 1025])
def test_sizes_at_the_path_boundary(eng, n):
    """The largest matrix whose bits sit in LDS (the kernel's biggest LDS request) and the smallest that goes to device memory,
    against the restatement."""
    from pyani_amd import classify
    I, C = cc.family_matrices(n=n, seed=21, families=9, subfamilies=3)
    seq = classify.classify(I, C, resolution=2e-3, memberships="special", engine=eng)
    want, parts = cc.restate(I, C, resolution=2e-3, partitions=True)
    assert_tuples(as_tuples(seq), want, f"n = {n}")
    assert any(s.membership for s in seq)
    for s, p in zip(seq, parts):
        if s.membership is not None:
            assert partition_of(s.membership) == p


def test_run_anim_then_classify_run(eng, genome_dir, tmp_path):
    """A real run on committed fixture genomes, then classify_run on its stored strings: equal to the restatement on the PARSED
    strings (the reference classifies what read_json gives back, not the run's float matrices)."""
    import io
    import shutil
    import pandas as pd
    from pyani_amd import classify
    from pyani_amd.subcmd_anim import run_anim
    for path in list(genome_dir["blochmannia"].values())[:4]:
        shutil.copy(path, tmp_path / path.name)
    run = run_anim(tmp_path, engine=eng)
    seq = classify.classify_run(run, cov_min=0, id_min=0, memberships="all", engine=eng)
    I = pd.read_json(io.StringIO(run.json["df_identity"])).to_numpy(dtype=np.float64)
    C = pd.read_json(io.StringIO(run.json["df_coverage"])).to_numpy(dtype=np.float64)
    want, parts = cc.restate(I, C, cov_min=0, id_min=0, partitions=True)
    assert_tuples(as_tuples(seq), want, "run_anim + classify_run")
    labels = [f"Genome_id:{g}" for g in sorted(run.genome_ids.values())]
    for s, p in zip(seq, parts):
        assert partition_of(s.membership) == {frozenset(labels[g] for g in comp) for comp in p}
    assert as_tuples(classify.classify_run(run.json, cov_min=0, id_min=0, memberships="none", engine=eng)) == as_tuples(seq)


def test_profile_slots_report_one_launch_each(eng):
    from pyani_amd import _lib, classify
    I, C, labels = cc.build_case("n60_default")
    eng.profile_enable(True)
    eng.profile_config()
    eng.profile_reset()
    try:
        classify.classify(I, C, labels, resolution=1e-3, memberships="none", engine=eng)
        (ms_e, n_e), (ms_s, n_s) = eng.profile_get(_lib.K_CLASSIFY_EDGE), eng.profile_get(_lib.K_CLASSIFY_SWEEP)
    finally:
        eng.profile_enable(False)
        eng.profile_reset()
    assert (n_e, n_s) == (1, 1) and ms_e > 0 and ms_s > 0
    assert eng.kernel_name(_lib.K_CLASSIFY_EDGE) == "classify_edge_kernel"


def test_abi_errors(eng):
    from pyani_amd import _lib
    eng.classify_release()
    with pytest.raises(_lib.PyaniGpuError) as e:
        eng.classify_sweep([0.9, 1.0])
    assert e.value.code == _lib.PG_E_ARG and "pg_classify_edges" in str(e.value)
    I, C, _ = cc.build_case("n12_default")
    gold = load_gold("n12_default")
    assert eng.classify_edges(I, C) == (gold["n_edges"], gold["tuples"][0][1])
    with pytest.raises(_lib.PyaniGpuError):
        eng.classify_sweep([1.0, 0.9])
    with pytest.raises(_lib.PyaniGpuError):
        eng.classify_sweep([0.9, float("nan")])
    eng.classify_release()
    # over the supported size: an error with a text, never a truncation (the size check comes before any read of the matrices)
    assert eng.lib.pg_classify_edges(eng._h, I.ctypes.data, C.ctypes.data, 8193, 0.8, 0.5, None, None) == _lib.PG_E_ARG
    assert b"8192" in eng.lib.pg_last_error(eng._h)
