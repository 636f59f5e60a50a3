"""GPU: the heatmap clustering through the C ABI (pg_cluster_pdist / pg_cluster_linkage / pg_cluster_linkage_batch) reproduces every
golden case (tests/golden/heatmap) in both orientations: distances bit for bit (by SHA-1 where the golden holds only that), Z bit
for bit for "complete" and "average", leaves, ivl and the ordered frame equal; the batch call equals the single calls; the
reference's two ValueErrors are raised; 8193 observations are refused.  No case is skipped."""
import numpy as np
import pandas as pd
import pytest

from tests import heatmap_cases as hc
from tests.test_heatmap_cpu import ERROR_CASES, OK_CASES, problems_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


@pytest.mark.parametrize("name", OK_CASES)
def test_distances_equal_golden(eng, name):
    from pyani_amd import graphics
    meta, arrays = hc.load_gold(name)
    probs, _ = problems_of(name)
    for mat, o, key, frame in probs:
        rec = meta["matrices"][mat][o]
        x = np.ascontiguousarray(frame.to_numpy(dtype=np.float64))      # ONE matrix; the column orientation reads it in place
        d = eng.cluster_pdist(x, columns=(o == "col"))
        assert d.shape == (rec["n"] * (rec["n"] - 1) // 2,)
        assert hc.sha1(d) == rec["dist_sha1"], f"{name} {key}: distances differ from scipy's"
        if f"{key}|dist" in arrays:
            assert hc.same_bits(d, arrays[f"{key}|dist"])
        assert hc.same_bits(d, graphics.pdist(frame, columns=(o == "col"), engine=eng))


@pytest.mark.parametrize("method", hc.METHODS)
@pytest.mark.parametrize("name", OK_CASES)
def test_linkage_leaves_labels_and_frame_equal_golden(eng, name, method):
    from pyani_amd import _lib, graphics
    meta, arrays = hc.load_gold(name)
    probs, labels = problems_of(name)
    frames, _ = hc.build_case(name)
    code = {"complete": _lib.PG_CLUSTER_COMPLETE, "average": _lib.PG_CLUSTER_AVERAGE}[method]
    singles = {}
    for mat, o, key, frame in probs:
        x = np.ascontiguousarray(frame.to_numpy(dtype=np.float64))
        merges = eng.cluster_linkage(x, method=code, columns=(o == "col"))
        singles[key] = merges
        Z = graphics.merges_to_linkage(merges)
        assert hc.same_bits(Z, hc.gold_z(arrays, key, method)), f"{name} {key} {method}: Z differs from scipy's"
        assert hc.same_bits(Z, graphics.linkage(frame, method=method, columns=(o == "col"), engine=eng))
        assert graphics.dendrogram_leaves(Z) == arrays[f"{key}|{method}|leaves"].tolist()
        assert graphics.dendrogram_labels(Z, labels) == meta["matrices"][mat][o][method]["ivl"]
    # the batched call: the same records as the single calls, and everything heatmap() needs
    got = graphics.run_heatmap_orders(frames, method=method, labels=labels, engine=eng)
    mats = {mat: np.ascontiguousarray(frame.to_numpy(dtype=np.float64)) for mat, o, _, frame in probs if o == "row"}
    batch = eng.cluster_linkage_batch([(mats[mat], o == "col", code) for mat, o, _, _ in probs])
    for (mat, o, key, frame), merges in zip(probs, batch):
        assert hc.same_bits(merges, singles[key]), f"{name} {key} {method}: batch and single call differ"
    for mat, f in frames.items():
        frame = hc.as_frame(f).sort_index()
        rl, cl = (arrays[f"{mat}|{o}|{method}|leaves"].tolist() for o in hc.ORIENTATIONS)
        g = got[mat] if len(frames) > 1 else graphics.heatmap_order(f, method=method, labels=labels, engine=eng)
        assert (g.row_leaves, g.col_leaves) == (rl, cl)
        assert g.row_ivl == meta["matrices"][mat]["row"][method]["ivl"] and g.col_ivl == meta["matrices"][mat]["col"][method]["ivl"]
        assert hc.same_bits(g.row_linkage, hc.gold_z(arrays, f"{mat}|row", method))
        assert hc.same_bits(g.col_linkage, hc.gold_z(arrays, f"{mat}|col", method))
        pd.testing.assert_frame_equal(g.frame, frame.iloc[rl, cl], check_exact=True)
        pd.testing.assert_frame_equal(got[mat].frame, g.frame, check_exact=True)


@pytest.mark.parametrize("name", ERROR_CASES)
def test_value_errors(eng, name):
    from pyani_amd import _lib, graphics
    meta, _ = hc.load_gold(name)
    assert meta["raises"] == "ValueError"
    frames, labels = hc.build_case(name)
    for method in hc.METHODS:
        with pytest.raises(ValueError):
            graphics.heatmap_order(frames["m"], method=method, labels=labels, engine=eng)
        with pytest.raises(ValueError):
            graphics.linkage(frames["m"], method=method, engine=eng)
    x = np.ascontiguousarray(frames["m"].to_numpy(dtype=np.float64))
    if len(x) >= 2:      # the NaN cell, at the ABI: its own status code, in single and batch calls, and only for the problem it is in
        with pytest.raises(_lib.PyaniGpuError) as e:
            eng.cluster_linkage(x)
        assert e.value.code == _lib.PG_E_NONFINITE
        with pytest.raises(ValueError):
            graphics.pdist(x, engine=eng)
        good = np.ascontiguousarray(hc.build_case("n12")[0]["m"].to_numpy(dtype=np.float64))
        out = eng.cluster_linkage_batch([(good, False, 0), (x, False, 0), (good, True, 1)])
        assert out[1] is None and out[0] is not None and out[2] is not None
        assert hc.same_bits(out[0], eng.cluster_linkage(good))
    else:        # one observation: refused at the ABI too
        with pytest.raises(_lib.PyaniGpuError) as e:
            eng.cluster_linkage(x)
        assert e.value.code == _lib.PG_E_ARG


def test_overflow_to_infinity_is_refused(eng):
    from pyani_amd import graphics
    x = np.zeros((3, 2))
    x[0, 0], x[1, 0] = 1e200, -1e200
    with pytest.raises(ValueError):
        graphics.linkage(x, engine=eng)


def test_more_than_8192_observations_are_refused(eng):
    from pyani_amd import _lib
    x = np.zeros((4, 4))      # the size check comes before any read of the matrix
    assert eng.lib.pg_cluster_linkage(eng._h, x.ctypes.data, 8193, 4, 0, 0, x.ctypes.data) == _lib.PG_E_ARG
    assert b"8192" in eng.lib.pg_last_error(eng._h)
    assert eng.lib.pg_cluster_pdist(eng._h, x.ctypes.data, 4, 8193, 1, x.ctypes.data) == _lib.PG_E_ARG
    assert b"8192" in eng.lib.pg_last_error(eng._h)


def test_long_observations_and_profile_slots(eng):
    """The observation length is unbounded: 5 observations of 20 001 elements, both orientations of one matrix, against the
    restatement; and the two profile slots count their launches."""
    from pyani_amd import _lib, graphics
    with np.errstate(over="ignore"):
        h = hc.splitmix64(np.arange(5 * 20001, dtype=hc.U) + hc.U(99)).reshape(5, 20001)
    x = (h % hc.U(1000003)).astype(np.float64) / 977.0
    eng.profile_enable(True)
    eng.profile_config()
    eng.profile_reset()
    try:
        d = eng.cluster_pdist(x)
        dt = eng.cluster_pdist(np.ascontiguousarray(x.T), columns=True)
        Z = graphics.linkage(x, method="average", engine=eng)
        (ms_p, n_p), (ms_l, n_l) = eng.profile_get(_lib.K_CLUSTER_PDIST), eng.profile_get(_lib.K_CLUSTER_LINKAGE)
    finally:
        eng.profile_enable(False)
        eng.profile_reset()
    want = hc.restate_pdist(x)
    assert hc.same_bits(d, want) and hc.same_bits(dt, want)
    assert hc.same_bits(Z, hc.restate_label(hc.restate_chain(want, 5, "average")))
    assert (n_p, n_l) == (3, 1) and ms_p > 0 and ms_l > 0
    assert eng.kernel_name(_lib.K_CLUSTER_PDIST) == "cluster_pdist_kernel"
