"""CPU-only: the distribution plots' goldens (tests/golden/distribution, tools/make_distribution_goldens.py: the reference's own
distribution() for "mpl", numpy's and scipy's answers to seaborn's calls for "seaborn") against (a) the test-only numpy restatement
of tests/distribution_cases.py, edges, counts, support and bandwidth exactly and the density within the derived bound, for every
case, and (b) the PRODUCT's host pieces (pyani_amd.graphics: bin edges, grid, bandwidth, normalisation, errors) with the device
replaced by a numpy stub.  The bandwidth is held to scipy's own value computed in the test's process (its last bits depend on the
BLAS's threads, tests/distribution_cases.py) and that value to the golden's within a rounding bound.  No matplotlib or reference at
test time."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import distribution_cases as dc

ROOT = Path(__file__).resolve().parent.parent
LEGS = [(c, m) for c in dc.CASES for m in dc.METHODS]
OK_LEGS = [(c, m) for c, m in LEGS if not dc.raises_of(c, m)]
ERROR_LEGS = [(c, m) for c, m in LEGS if dc.raises_of(c, m)]


def test_every_case_has_a_golden_and_nothing_else():
    assert sorted(p.stem for p in dc.GOLDEN_DIR.glob("*.npz")) == sorted(dc.CASES)
    assert len(ERROR_LEGS) == 5 and len(OK_LEGS) >= 23
    sizes = {dc.flat(f).size for c in ("n2", "n12", "n63", "n64", "n65", "n1000_clipped") for f in dc.build_case(c).values()}
    assert sizes == {4, 144, 63 * 63, 64 * 64, 65 * 65, 1000 * 1000}
    assert len(dc.build_case("n12_run_json")) == 5 and all(isinstance(f, str) for f in dc.build_case("n12_run_json").values())


def test_cases_are_what_they_claim():
    x = dc.flat(dc.build_case("n1000_clipped")["m"])
    assert x.max() == 1.0 and (x == 1.0).sum() > 20000 and not np.array_equal(x.reshape(1000, 1000), x.reshape(1000, 1000).T)
    assert (dc.flat(dc.build_case("n200_coverage_zeros")["m"]) == 0.0).sum() > 1000
    assert dc.flat(dc.build_case("n200_aln_lengths")["m"]).max() > 5e6
    f = dc.build_case("n200_sim_errors")["m"]
    assert all(np.issubdtype(t, np.integer) for t in f.dtypes)
    x = dc.flat(dc.build_case("n150_two_decimals")["m"])
    assert np.array_equal(x, np.round(x, 2)) and len(np.unique(x)) < 40
    assert np.isnan(dc.flat(dc.build_case("n12_nan_cell")["m"])).sum() == 1
    assert len(np.unique(dc.flat(dc.build_case("n20_all_equal")["m"]))) == 1 and dc.flat(dc.build_case("n1_single")["m"]).size == 1


@pytest.mark.parametrize("name,method", OK_LEGS)
def test_restatement_reproduces_golden(name, method):
    meta, arrays = dc.load_gold(name)
    frames = dc.build_case(name)
    assert sorted(meta["matrices"]) == sorted(frames)
    for mat, f in frames.items():
        x = dc.flat(f)
        rec = meta["matrices"][mat]
        assert rec["n"] == x.size and rec[method]["raises"] is None
        assert rec[method]["n_used"] == int((~np.isnan(x)).sum())
        dc.check_against_gold(name, method, mat, arrays, x, dc.restate(x, method))


@pytest.mark.parametrize("name,method", ERROR_LEGS)
def test_error_cases_are_what_they_claim(name, method):
    meta, arrays = dc.load_gold(name)
    for mat, f in dc.build_case(name).items():
        assert meta["matrices"][mat][method]["raises"] == dc.raises_of(name, method)
        assert not any(k.startswith(f"{mat}|{method}|") for k in arrays)
        with pytest.raises(dc.EXCEPTIONS[dc.raises_of(name, method)]):
            dc.restate(dc.flat(f), method)


def test_seaborn_leg_says_it_is_not_a_run_of_seaborn():
    meta, _ = dc.load_gold("n12")
    assert "not the reference's own run" in meta["provenance"]["seaborn"] and "reference's own" in meta["provenance"]["mpl"]


@pytest.mark.parametrize("name,method", OK_LEGS)
def test_product_host_pieces_reproduce_golden(name, method):
    from pyani_amd import graphics
    meta, arrays = dc.load_gold(name)
    frames = dc.build_case(name)
    eng = dc.HostEngine()
    got = graphics.run_distributions(frames, method=method, engine=eng)
    assert list(got) == list(frames) and eng.loads == len(frames) and eng.releases == 1      # each matrix uploaded once
    for mat, f in frames.items():
        g = got[mat]
        assert isinstance(g, graphics.DistributionData) and g._fields == ("bin_edges", "counts", "support", "density", "bandwidth")
        x = dc.flat(f)
        dc.check_against_gold(name, method, mat, arrays, x, g)
        if dc.flat(f).size <= 100000:      # (the stub's density is slow on the large case)
            one = graphics.distribution_data(f, method=method, engine=dc.HostEngine())
            assert all(dc.same_bits(a, b) for a, b in zip(one, g))
        assert dc.same_bits(graphics.scott_bandwidth(x[~np.isnan(x)])[0], g.bandwidth)


@pytest.mark.parametrize("name,method", ERROR_LEGS)
def test_product_raises_the_golden_errors(name, method):
    from pyani_amd import graphics
    for f in dc.build_case(name).values():
        eng = dc.HostEngine()
        with pytest.raises(dc.EXCEPTIONS[dc.raises_of(name, method)]):
            graphics.distribution_data(f, method=method, engine=eng)
        assert eng.releases == 1 and eng.x is None      # nothing stays resident after a refusal


def test_refusals_and_inputs_need_no_device():
    from pyani_amd import graphics
    with pytest.raises(ValueError):
        graphics.distribution_data(np.ones((3, 3)), method="plotly", engine=dc.HostEngine())
    with pytest.raises(ValueError):
        graphics.run_distributions({"m": np.ones((3, 3))}, method="plotly", engine=dc.HostEngine())
    with pytest.raises(ValueError):      # an infinite cell: hist() refuses the range, gaussian_kde the value
        graphics.distribution_data(np.array([[1.0, np.inf], [0.5, 0.25]]), engine=dc.HostEngine())
    with pytest.raises(ValueError):
        graphics.distribution_data(np.array([[1.0, np.inf], [0.5, 0.25]]), method="seaborn", engine=dc.HostEngine())
    with pytest.raises(ValueError):
        graphics.distribution_data(np.full((2, 2), np.nan), method="seaborn", engine=dc.HostEngine())
    # arrays, frames and JSON strings of one matrix give one answer; the frame is NOT sorted (the values' order is the reference's)
    f = dc.build_case("n12")["m"].iloc[::-1]
    a = graphics.distribution_data(f, engine=dc.HostEngine())
    assert all(dc.same_bits(u, v) for u, v in zip(a, graphics.distribution_data(f.to_numpy(), engine=dc.HostEngine())))
    assert dc.same_bits(a.bandwidth, dc.restate_bandwidth(f.to_numpy().reshape(-1))[0])
    s = dc.build_case("n12_run_json")["df_identity"]
    a = graphics.distribution_data(s, engine=dc.HostEngine())
    assert all(dc.same_bits(u, v) for u, v in zip(a, graphics.distribution_data(dc.as_frame(s), engine=dc.HostEngine())))


def test_equal_extremes_get_numpys_half_widening():
    """min == max with a positive bandwidth cannot come from data (the covariance is singular), so the rule is checked on the edges
    alone: numpy widens the range by 0.5 on both sides."""
    e = np.histogram_bin_edges(np.empty(0), bins=50, range=(0.75, 0.75))
    assert dc.same_bits(e, np.linspace(0.25, 1.25, 51))


def test_tolerance_is_the_derived_one():
    assert dc.density_tolerance(10 ** 6, 1.0) == (10 ** 6 * 2.0 ** -53 + 2.0 ** -40) * 1.0 + 1e-300
    assert 1.0e-10 < dc.density_tolerance(10 ** 6, 1.0) < 1.2e-10


def test_abi_has_the_dist_calls_and_no_new_slot():
    from pyani_amd import build, _lib
    build.build_gpu()
    lib = _lib.load()
    header = (ROOT / "include" / "pyani_gpu.h").read_text()
    for sym in ("pg_dist_load", "pg_dist_hist", "pg_dist_kde", "pg_dist_release", "pg_dist_last_ms"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert (_lib.K_COUNT, _lib.K_TOTAL) == (18, 20)
    assert re.search(r"#define PG_K__COUNT 20\b", header) and lib.pg_kernel_name(20) == b""
    import ctypes
    assert ctypes.sizeof(_lib.DistStats) == 32
    from pyani_amd.engine import Engine
    for m in ("dist_load", "dist_hist", "dist_kde", "dist_release", "dist_last_ms"):
        assert callable(getattr(Engine, m))
