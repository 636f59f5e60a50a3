"""GPU: the distribution plots through the C ABI (pg_dist_load / pg_dist_hist / pg_dist_kde) reproduce every golden case
(tests/golden/distribution) for both methods: counts and bin edges equal exactly; the bandwidth equal bit for bit to scipy's own on
the same values in this process and within a rounding bound of the golden's (scipy's last bits change with the BLAS's threads:
tests/distribution_cases.py), the support accordingly; the density within the derived bound (density_tolerance there) of scipy's
stored value AND of the high-precision one; the reference's errors are raised.  Two calls give identical bits; run_distributions equals the single calls; the limits are refused with
PG_E_ARG; uneven edges agree with np.histogram; values outside the edges are not counted.  No case is skipped."""
import numpy as np
import pytest

from tests import distribution_cases as dc
from tests.test_distribution_cpu import ERROR_LEGS, OK_LEGS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    with Engine(0) as e:
        yield e


@pytest.mark.parametrize("name,method", OK_LEGS)
def test_distribution_equals_golden(eng, name, method):
    from pyani_amd import graphics
    meta, arrays = dc.load_gold(name)
    frames = dc.build_case(name)
    singles = {}
    for mat, f in frames.items():
        g = graphics.distribution_data(f, method=method, engine=eng)
        dc.check_against_gold(name, method, mat, arrays, dc.flat(f), g)
        again = graphics.distribution_data(f, method=method, engine=eng)
        assert all(dc.same_bits(a, b) for a, b in zip(g, again)), f"{name} {mat} {method}: two calls differ"
        singles[mat] = g
    got = graphics.run_distributions(frames, method=method, engine=eng)
    assert list(got) == list(frames)
    for mat in frames:
        assert all(dc.same_bits(a, b) for a, b in zip(got[mat], singles[mat])), f"{name} {mat} {method}: run and single call differ"


@pytest.mark.parametrize("name,method", ERROR_LEGS)
def test_reference_errors_are_raised(eng, name, method):
    from pyani_amd import graphics
    for f in dc.build_case(name).values():
        with pytest.raises(dc.EXCEPTIONS[dc.raises_of(name, method)]):
            graphics.distribution_data(f, method=method, engine=eng)


def test_stats_are_exact(eng):
    x = dc.flat(dc.build_case("n65")["m"]).copy()
    x[[5, 77, 4000]] = np.nan
    x[[9, 1234]] = [np.inf, -np.inf]
    assert eng.dist_load(x) == (-np.inf, np.inf, 3, 2)
    x[[9, 1234]] = np.nan
    ok = x[~np.isnan(x)]
    assert eng.dist_load(x) == (ok.min(), ok.max(), 5, 0)
    assert eng.dist_load(np.full(130, np.nan)) == (np.inf, -np.inf, 130, 0)
    big = dc.flat(dc.build_case("n1000_clipped")["m"])
    assert eng.dist_load(big) == (big.min(), big.max(), 0, 0)
    eng.dist_release()


def test_density_bits_do_not_change_between_calls(eng):
    from pyani_amd import graphics
    x = dc.flat(dc.build_case("n1000_clipped")["m"])
    lo, hi, _, _ = eng.dist_load(x)
    bw = graphics.scott_bandwidth(x)[0]
    for m in (1, 64, 200, 1024):
        p = np.linspace(lo, hi, m)
        a, b = eng.dist_kde(p, bw), eng.dist_kde(p, bw)
        assert dc.same_bits(a, b) and (a > 0).all()
    # a point's sum does not depend on how many points share the launch
    assert dc.same_bits(eng.dist_kde(np.linspace(lo, hi, 200), bw)[:1], eng.dist_kde(np.array([lo]), bw))
    eng.dist_release()


def test_kde_skips_nan_and_matches_numpy_on_a_small_set(eng):
    x = dc.flat(dc.build_case("n64")["m"]).copy()
    x[::7] = np.nan
    ok = x[~np.isnan(x)]
    eng.dist_load(x)
    p = np.linspace(0.7, 1.05, 200)
    got = eng.dist_kde(p, 0.01)
    want = dc.restate_density(ok, p, 0.01) * len(ok) / (np.power(2 * np.pi, -0.5) / 0.01)
    assert dc.density_close(got, want, len(ok))
    eng.dist_release()


def test_limits_are_refused(eng):
    from pyani_amd import _lib

    def refused(call):
        with pytest.raises(_lib.PyaniGpuError) as err:
            call()
        assert err.value.code == _lib.PG_E_ARG

    eng.dist_release()
    refused(lambda: eng.dist_hist(np.linspace(0, 1, 51)))      # nothing loaded
    refused(lambda: eng.dist_kde(np.linspace(0, 1, 200), 0.1))
    # one value more than 8192 x 8192: refused on the count alone, before anything is read (one page backs the argument)
    one = np.zeros(1, dtype=np.float64)
    st = _lib.DistStats()
    import ctypes
    assert eng.lib.pg_dist_load(eng._h, one.ctypes.data, 8192 * 8192 + 1, ctypes.addressof(st)) == _lib.PG_E_ARG
    refused(lambda: eng.dist_load(np.zeros(0)))
    eng.dist_load(np.linspace(0.0, 1.0, 1000))
    refused(lambda: eng.dist_hist(np.linspace(0, 1, 4098)))      # 4097 bins
    assert eng.dist_hist(np.linspace(0, 1, 4097)).sum() == 1000  # 4096 bins
    refused(lambda: eng.dist_kde(np.linspace(0, 1, 1025), 0.1))
    assert eng.dist_kde(np.linspace(0, 1, 1024), 0.1).shape == (1024,)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(lambda: eng.dist_kde(np.linspace(0, 1, 200), bad))
    refused(lambda: eng.dist_hist(np.array([0.0, 0.5, 0.4, 1.0])))
    refused(lambda: eng.dist_hist(np.array([0.0, np.nan, 1.0])))
    eng.dist_release()
    refused(lambda: eng.dist_hist(np.linspace(0, 1, 51)))


@pytest.mark.parametrize("name", ["n1000_clipped", "n150_two_decimals", "n200_coverage_zeros", "n200_sim_errors"])
def test_uneven_and_partial_edges_agree_with_numpy(eng, name):
    x = dc.flat(dc.build_case(name)["m"]).copy()
    x[::1001] = np.nan
    lo, hi, _, _ = eng.dist_load(x)
    ok = x[~np.isnan(x)]
    q = np.unique(np.quantile(ok, np.linspace(0, 1, 38)))
    grids = [q,                                                     # uneven, ties on edges
             np.concatenate([[lo], lo + (hi - lo) * np.linspace(0.001, 1, 300) ** 3]),      # uneven, 300 bins
             np.linspace(lo + (hi - lo) * 0.25, lo + (hi - lo) * 0.75, 41),      # even, values outside on both sides
             np.array([lo + (hi - lo) * 0.5, hi]),                  # one bin
             np.array([hi, hi + 1.0]), np.array([lo - 1.0, lo]),    # only the extreme cells, on a left and on a right edge
             np.array([lo, lo, (lo + hi) / 2, (lo + hi) / 2, hi, hi]),      # equal neighbours
             np.linspace(lo, hi, 4097),
             np.round(np.linspace(lo, hi, 101), 2) if name == "n150_two_decimals" else np.linspace(lo, hi, 1000)]
    for edges in grids:
        want = np.histogram(ok, edges)[0]
        got = eng.dist_hist(edges)
        assert got.dtype == np.int64 and np.array_equal(got, want), f"{name}: {len(edges) - 1} bins from {edges[0]} to {edges[-1]}"
    assert eng.dist_hist(np.array([hi + 1.0, hi + 2.0])).sum() == 0 and eng.dist_hist(np.array([lo - 2.0, lo - 1.0])).sum() == 0
    eng.dist_release()


def test_last_ms_follows_the_profile_switch(eng):
    x = dc.flat(dc.build_case("n1000_clipped")["m"])
    eng.profile_enable(False)
    lo, hi, _, _ = eng.dist_load(x)
    eng.dist_hist(np.linspace(lo, hi, 51))
    assert eng.dist_last_ms() == (0.0, 0.0, 0.0)
    eng.profile_enable(True)
    try:
        eng.dist_load(x)
        eng.dist_hist(np.linspace(lo, hi, 51))
        eng.dist_kde(np.linspace(lo, hi, 200), 0.01)
        ms = eng.dist_last_ms()
        assert all(0.0 < t < 10000.0 for t in ms), ms
    finally:
        eng.profile_enable(False)
        eng.dist_release()
    assert eng.dist_last_ms() == (0.0, 0.0, 0.0)
