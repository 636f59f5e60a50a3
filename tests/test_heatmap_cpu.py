"""CPU-only: the heatmap clustering's goldens (tests/golden/heatmap, tools/make_heatmap_goldens.py: the reference's own
add_dendrogram for "complete", scipy's answer to clustermap's calls for "average") against (a) the test-only numpy restatement of
tests/heatmap_cases.py, distances, linkage, leaves and labels, bit for bit, for every case, and (b) the PRODUCT's host pieces
(pyani_amd.graphics: stable sort + relabelling, leaf traversal, labels, the sort_index rule), which must turn the golden merge
records into the golden Z, leaves, ivl and ordered frame.  No scipy, matplotlib or reference at test time."""
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import heatmap_cases as hc

ROOT = Path(__file__).resolve().parent.parent
OK_CASES = [c for c in hc.CASES if not hc.CASES[c].get("raises")]
ERROR_CASES = [c for c in hc.CASES if hc.CASES[c].get("raises")]


def problems_of(name):
    """[(matrix name, orientation, key, row-sorted frame)] of a case."""
    frames, labels = hc.build_case(name)
    out = []
    for mat, f in frames.items():
        frame = hc.as_frame(f).sort_index()
        out += [(mat, o, f"{mat}|{o}", frame) for o in hc.ORIENTATIONS]
    return out, labels


def test_every_case_has_a_golden_and_nothing_else():
    assert sorted(p.stem for p in hc.GOLDEN_DIR.glob("*.npz")) == sorted(hc.CASES)
    assert len(ERROR_CASES) == 2 and len(OK_CASES) >= 19


@pytest.mark.parametrize("name", OK_CASES)
def test_restatement_reproduces_golden(name):
    meta, arrays = hc.load_gold(name)
    assert meta["raises"] is None
    probs, labels = problems_of(name)
    assert len(probs) == 2 * len(meta["matrices"])
    for mat, o, key, frame in probs:
        rec = meta["matrices"][mat][o]
        X = hc.observations(frame, o)
        assert X.shape == (rec["n"], rec["m"])
        dists = hc.restate_pdist(X)
        assert hc.sha1(dists) == rec["dist_sha1"], f"{name} {key}: distances"
        assert (f"{key}|dist" in arrays) == (rec["n"] <= hc.FULL_DISTANCES_UP_TO)
        if f"{key}|dist" in arrays:
            assert hc.same_bits(dists, arrays[f"{key}|dist"]), f"{name} {key}: distances"
        for method in hc.METHODS:
            merges = hc.restate_chain(dists, rec["n"], method)
            assert hc.same_bits(merges, hc.gold_z(arrays, key, method, "M")), f"{name} {key} {method}: merge records"
            Z = hc.restate_label(merges)
            assert hc.same_bits(Z, hc.gold_z(arrays, key, method)), f"{name} {key} {method}: Z"
            leaves = hc.restate_leaves(Z)
            assert leaves == arrays[f"{key}|{method}|leaves"].tolist()
            assert hc.restate_ivl(leaves, labels) == rec[method]["ivl"]


@pytest.mark.parametrize("name", ERROR_CASES)
def test_error_cases_are_what_they_claim(name):
    meta, arrays = hc.load_gold(name)
    assert meta["raises"] == "ValueError" and not arrays
    probs, _ = problems_of(name)
    X = hc.observations(probs[0][3], "row")
    assert len(X) < 2 or not np.isfinite(hc.restate_pdist(X)).all()


class GoldenEngine:
    """Stands in for the device: hands back the golden merge records, and checks what it is asked."""

    def __init__(self, arrays, keys, expect):
        self.arrays, self.keys, self.expect, self.calls = arrays, keys, expect, 0

    def cluster_linkage_batch(self, problems):
        from pyani_amd import _lib
        self.calls += 1
        assert len(problems) == len(self.keys)
        out = []
        for (x, columns, code), (key, method), want in zip(problems, self.keys, self.expect):
            assert code == {"complete": _lib.PG_CLUSTER_COMPLETE, "average": _lib.PG_CLUSTER_AVERAGE}[method]
            assert np.asarray(x).flags.c_contiguous      # what the C call is given; either orientation of it may be asked for
            assert hc.same_bits(x if not columns else np.asarray(x).T, want)
            out.append(hc.gold_z(self.arrays, key, method, "M"))
        return out


@pytest.mark.parametrize("method", hc.METHODS)
@pytest.mark.parametrize("name", OK_CASES)
def test_product_host_pieces_reproduce_golden(name, method):
    from pyani_amd import graphics
    meta, arrays = hc.load_gold(name)
    probs, labels = problems_of(name)
    for mat, o, key, frame in probs:
        Z = graphics.merges_to_linkage(hc.gold_z(arrays, key, method, "M"))
        assert hc.same_bits(Z, hc.gold_z(arrays, key, method)), f"{name} {key} {method}: Z"
        assert graphics.dendrogram_leaves(Z) == arrays[f"{key}|{method}|leaves"].tolist()
        assert graphics.dendrogram_labels(Z, labels) == meta["matrices"][mat][o][method]["ivl"]
    # the whole host path, the device replaced by the golden records: one batched call, the frame sorted by ROW index only
    frames, _ = hc.build_case(name)
    keys = [(key, method) for _, _, key, _ in probs]
    eng = GoldenEngine(arrays, keys, [hc.observations(frame, o) for _, o, _, frame in probs])
    got = graphics.run_heatmap_orders(frames, method=method, labels=labels, engine=eng)
    assert eng.calls == 1 and list(got) == list(frames)
    for mat, f in frames.items():
        frame = hc.as_frame(f).sort_index()
        rl, cl = (arrays[f"{mat}|{o}|{method}|leaves"].tolist() for o in hc.ORIENTATIONS)
        g = got[mat]
        assert (g.row_leaves, g.col_leaves) == (rl, cl)
        assert g.row_ivl == meta["matrices"][mat]["row"][method]["ivl"] and g.col_ivl == meta["matrices"][mat]["col"][method]["ivl"]
        assert hc.same_bits(g.row_linkage, hc.gold_z(arrays, f"{mat}|row", method))
        assert hc.same_bits(g.col_linkage, hc.gold_z(arrays, f"{mat}|col", method))
        pd.testing.assert_frame_equal(g.frame, frame.iloc[rl, cl], check_exact=True)
    if len(frames) == 1:
        one = graphics.heatmap_order(frames["m"], method=method, labels=labels,
                                     engine=GoldenEngine(arrays, keys, [hc.observations(frame, o) for _, o, _, frame in probs]))
        assert one.row_leaves == got["m"].row_leaves and one.col_ivl == got["m"].col_ivl


def test_scrambled_index_case_really_is_scrambled():
    frames, _ = hc.build_case("n30_scrambled_index")
    f = frames["m"]
    assert list(f.index) != sorted(f.index) and list(f.columns) == sorted(f.columns)


def test_deep_chain_tree_needs_no_recursion():
    from pyani_amd import graphics
    n = 8192      # every merge joins the next leaf to the cluster so far: depth n - 1
    merges = np.array([[k, k + 1, float(k + 1), k + 2] for k in range(n - 1)], dtype=np.float64)
    Z = graphics.merges_to_linkage(merges)
    assert hc.same_bits(Z, hc.restate_label(merges))
    leaves = graphics.dendrogram_leaves(Z)
    assert leaves == hc.restate_leaves(Z) and sorted(leaves) == list(range(n))
    assert graphics.dendrogram_labels(Z)[:2] == [str(leaves[0]), str(leaves[1])]


def test_stable_sort_keeps_tied_heights_in_merge_order():
    from pyani_amd import graphics
    merges = np.array([[2, 3, 1.0, 2], [0, 1, 1.0, 2], [1, 3, 2.0, 4]], dtype=np.float64)
    assert graphics.merges_to_linkage(merges).tolist() == [[2, 3, 1.0, 2], [0, 1, 1.0, 2], [4, 5, 2.0, 4]]


def test_refusals_need_no_device():
    from pyani_amd import graphics
    with pytest.raises(ValueError):
        graphics.linkage(np.ones((1, 5)), engine=object())
    with pytest.raises(ValueError):
        graphics.heatmap_order(pd.DataFrame(np.ones((1, 1))), engine=object())
    with pytest.raises(ValueError):
        graphics.linkage(np.ones((3, 3)), method="ward", engine=object())
    with pytest.raises(ValueError):      # scipy: "Dimensions of Z and labels must be consistent."
        graphics.dendrogram_labels(np.array([[0, 1, 1.0, 2]]), {"a": "x", "b": "y", "c": "z"})
    assert graphics.pdist(np.ones((1, 4)), engine=object()).shape == (0,)


def test_abi_has_the_cluster_calls_and_slots():
    from pyani_amd import build, _lib
    build.build_gpu()
    lib = _lib.load()
    header = (ROOT / "include" / "pyani_gpu.h").read_text()
    for sym in ("pg_cluster_pdist", "pg_cluster_linkage", "pg_cluster_linkage_batch"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert (_lib.K_CLUSTER_PDIST, _lib.K_CLUSTER_LINKAGE, _lib.K_TOTAL) == (18, 19, 20)
    assert _lib.K_COUNT == 18      # the existing slots' count keeps its published value
    assert re.search(r"#define PG_K_CLUSTER_PDIST 18\b", header) and re.search(r"#define PG_K_CLUSTER_LINKAGE 19\b", header)
    assert re.search(r"#define PG_K__COUNT 20\b", header)
    assert lib.pg_kernel_name(18) == b"cluster_pdist_kernel" and lib.pg_kernel_name(19) == b"cluster_linkage_kernel"
    assert lib.pg_kernel_name(17) == b"classify_death_kernel+classify_sweep_kernel" and lib.pg_kernel_name(20) == b""
    import ctypes
    assert ctypes.sizeof(_lib.ClusterProblem) == 40
