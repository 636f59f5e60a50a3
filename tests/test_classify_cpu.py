"""CPU-only checks of the classify stage against the goldens the reference's own code produced (tools/make_classify_goldens.py):
the test-only restatement (tests/classify_cases.py) reproduces every tuple and every stored partition, the generator's bytes are
the ones the goldens were made from, pyani_amd.classify.break_thresholds gives the reference's intervals bit for bit in both break
modes, and classify() refuses to run without a device."""
import gzip
import json
from pathlib import Path

import numpy as np
import pytest

from tests import classify_cases as cc

GOLD = Path(__file__).resolve().parent / "golden" / "classify"


def load_gold(name):
    with gzip.open(GOLD / f"{name}.json.gz", "rt") as fh:
        return json.load(fh)


def case_inputs(name, gold):
    """The matrices the reference classified: the generator's, or for the JSON case the parsed strings."""
    if "json" in gold:
        import io
        import pandas as pd
        return (pd.read_json(io.StringIO(gold["json"]["df_identity"])).to_numpy(dtype=np.float64),
                pd.read_json(io.StringIO(gold["json"]["df_coverage"])).to_numpy(dtype=np.float64))
    I, C, _ = cc.build_case(name)
    return I, C


def assert_tuples(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} steps, the reference has {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        assert cc.same_float(g[0], w[0]) and tuple(g[1:]) == tuple(w[1:]), f"{what}: step {k}: {tuple(g)} != reference {tuple(w)}"


def test_every_case_has_a_golden():
    assert sorted(p.name[:-8] for p in GOLD.glob("*.json.gz")) == sorted(cc.CASES)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_generator_bytes_match_goldens(name):
    gold = load_gold(name)
    I, C, labels = cc.build_case(name)
    assert cc.sha1_of(I, C) == gold["sha1"]
    if "identity_hex" in gold:
        assert I.tobytes().hex() == gold["identity_hex"] and C.tobytes().hex() == gold["coverage_hex"]
    if "json" not in gold:
        assert labels == gold["labels"]
    assert gold["params"] == cc.params(name)


def test_cases_cover_both_break_modes_and_node_set_quirks():
    res = cc.DEFAULTS["resolution"]
    for name in ("n12_default", "n60_default", "n60_coarse"):      # edge by edge: the intervals are edge identities, duplicates kept
        gold = load_gold(name)
        assert gold["n_edges"] < 1 / res and len(gold["tuples"]) <= gold["n_edges"]
    assert len(load_gold("n60_default")["tuples"]) == load_gold("n60_default")["n_edges"]      # lowest edge gone, one step each, the last
    coarse = [t[0] for t in load_gold("n60_coarse")["tuples"]]
    assert len(set(coarse)) < len(coarse) / 2, "the coarse case must have many tied edges"
    for name in ("n200_default", "n400_default", "n1000_default", "n1500_default"):      # arange: a constant step from the lowest remaining edge
        gold = load_gold(name)
        iv = [t[0] for t in gold["tuples"]]
        assert gold["n_edges"] - 1 >= 1 / gold["params"]["resolution"]
        assert abs((iv[1] - iv[0]) - gold["params"]["resolution"]) < 1e-12 and iv[-1] == 1
    first = load_gold("n1000_default")["tuples"][0][0]
    assert first != round(first, 4), "the large arange case must not start on a round number"
    assert load_gold("n60_last_isolated")["tuples"][0][1] == 59 and load_gold("n60_middle_isolated")["tuples"][0][1] == 60
    assert load_gold("n12_no_edge")["raises"] == "IndexError" and load_gold("n12_no_edge_min_id")["tuples"] == [[1, 11, 11, True]]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_reproduces_reference(name):
    gold = load_gold(name)
    I, C = case_inputs(name, gold)
    if gold["raises"]:
        with pytest.raises(IndexError):
            cc.restate(I, C, **gold["params"])
        return
    want_parts = gold.get("partitions")
    if want_parts is None:
        assert_tuples(cc.restate(I, C, **gold["params"]), gold["tuples"], name)
        return
    got, parts = cc.restate(I, C, partitions=True, **gold["params"])
    assert_tuples(got, gold["tuples"], name)
    for k, (p, w) in enumerate(zip(parts, want_parts)):
        assert p == {frozenset(c) for c in w}, f"{name}: partition of step {k} differs from networkx.connected_components"


@pytest.mark.parametrize("name", list(cc.CASES))
def test_break_thresholds_match_reference_intervals(name):
    """break_thresholds from the sorted edge identities (the edge rule restated here in numpy) gives the golden's number of edges and
    its intervals bit for bit, one non-decreasing theta per step, the last at least 1."""
    from pyani_amd.classify import break_thresholds
    gold = load_gold(name)
    I, C = case_inputs(name, gold)
    par = gold["params"]
    n = len(I)
    iu, ju = np.triu_indices(n, 1)
    with np.errstate(invalid="ignore"):
        wi = np.where(I[iu, ju] < I[ju, iu], I[iu, ju], I[ju, iu])
        wc = np.where(C[iu, ju] < C[ju, iu], C[iu, ju], C[ju, iu])
        ids = np.sort(wi[(wi > par["id_min"]) & (wc > par["cov_min"])])
    assert len(ids) == gold["n_edges"]
    if gold["raises"]:
        with pytest.raises(IndexError):
            break_thresholds(ids, par["min_id"], par["max_id"], par["resolution"])
        return
    intervals, theta = break_thresholds(ids, par["min_id"], par["max_id"], par["resolution"])
    assert len(intervals) == len(theta) == len(gold["tuples"])
    for k, (iv, t) in enumerate(zip(intervals, gold["tuples"])):
        assert cc.same_float(iv, t[0]), f"{name}: interval {k}: {iv!r} != reference {t[0]!r}"
    assert theta.dtype == np.float64 and (np.diff(theta) >= 0).all() and theta[-1] >= 1.0


def test_classify_without_device_raises():
    """No CPU fallback: where no engine can be created (no HIP device) classify() raises PyaniGpuError too; where one can, it runs."""
    from pyani_amd import _lib, classify, engine
    I, C, labels = cc.build_case("n12_default")
    try:
        eng = engine.Engine(0)
    except _lib.PyaniGpuError:
        engine._default[0] = None
        with pytest.raises(_lib.PyaniGpuError):
            classify.classify(I, C, labels)
        return
    with eng:
        assert len(classify.classify(I, C, labels, resolution=1e-3, engine=eng)) == len(load_gold("n12_default")["tuples"])


def test_public_surface():
    from pyani_amd import _lib, classify
    assert classify.Cliquesinfo._fields == ("n_nodes", "n_subgraphs", "all_k_complete")
    assert classify.SubgraphData._fields == ("interval", "cliqueinfo", "membership")
    for name in ("classify", "classify_run", "break_thresholds", "special_intervals", "write_classify_tab"):
        assert callable(getattr(classify, name))
    assert (_lib.K_CLASSIFY_EDGE, _lib.K_CLASSIFY_SWEEP, _lib.K_COUNT) == (16, 17, 18)
    lib = _lib.load()
    assert lib.pg_kernel_name(16) == b"classify_edge_kernel" and b"classify_sweep_kernel" in lib.pg_kernel_name(17)


def test_write_classify_tab(tmp_path):
    from pyani_amd.classify import Cliquesinfo, SubgraphData, special_intervals, write_classify_tab
    seq = [SubgraphData(0.8727070381, Cliquesinfo(12, 3, False), None), SubgraphData(1, Cliquesinfo(12, 12, True), {})]
    assert special_intervals(seq) == seq[1:]
    write_classify_tab(tmp_path / "c.tab", seq)
    lines = (tmp_path / "c.tab").read_text().splitlines()
    assert lines[0].split("\t") == ["interval", "n_nodes", "n_subgraphs", "all_k_complete"]
    assert lines[1].split("\t") == ["0.8727070381", "12", "3", "False"] and lines[2].split("\t") == ["1", "12", "12", "True"]
