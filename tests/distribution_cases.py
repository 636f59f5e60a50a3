"""Shared by the distribution tests and tools/make_distribution_goldens.py: the input generator of the golden cases, the golden file
format, the density's tolerance, and an independent numpy restatement of what the reference's distribution plots compute (matplotlib's
hist(bins=50) and scipy's gaussian_kde on a 200-point grid; the numpy / scipy calls seaborn's histplot and kdeplot make) for tests only.

Inputs are made by integer hashing (tests/classify_cases.py: splitmix64, family_matrices), so the tests and the tool build identical
bytes on any numpy and only RESULTS are stored.  The restatement shares nothing with pyani_amd: it counts by sorting and searching
the edges, and sums the density in blocks of numpy calls."""
import json
from pathlib import Path

import numpy as np
import pandas as pd

from tests.classify_cases import U, family_matrices, splitmix64

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "distribution"
METHODS = ("mpl", "seaborn")
BINS, GRID, CUT = 50, 200, 3

# name -> how the matrices are made.  raises: the exception type per method (absent: none)
CASES = {
    "n2": dict(kind="ident", gen=dict(n=2, seed=61, families=1, subfamilies=1)),
    "n12": dict(kind="ident", gen=dict(n=12, seed=62, families=3, subfamilies=2)),
    "n63": dict(kind="ident", gen=dict(n=63, seed=63, families=4, subfamilies=3)),
    "n64": dict(kind="ident", gen=dict(n=64, seed=64, families=4, subfamilies=3)),
    "n65": dict(kind="ident", gen=dict(n=65, seed=65, families=4, subfamilies=3, asym=20000)),
    "n1000_clipped": dict(kind="ident", gen=dict(n=1000, seed=66, families=8, subfamilies=4, asym=30000), edits=["clip"]),
    "n200_coverage_zeros": dict(kind="coverage", gen=dict(n=200, seed=67, families=5, subfamilies=3)),
    "n200_aln_lengths": dict(kind="aln_lengths", gen=dict(n=200, seed=68, families=5, subfamilies=3)),
    "n200_sim_errors": dict(kind="sim_errors", gen=dict(n=200, seed=69, families=5, subfamilies=3)),
    "n150_two_decimals": dict(kind="ident", gen=dict(n=150, seed=70, families=4, subfamilies=3), edits=["round2"]),
    "n12_run_json": dict(kind="run", gen=dict(n=12, seed=71, families=3, subfamilies=2, asym=15000)),
    "n20_all_equal": dict(kind="equal", n=20, raises=dict(mpl="LinAlgError", seaborn="LinAlgError")),
    "n12_nan_cell": dict(kind="ident", gen=dict(n=12, seed=62, families=3, subfamilies=2), edits=["nan"], raises=dict(mpl="ValueError")),
    "n1_single": dict(kind="ident", gen=dict(n=1, seed=72, families=1, subfamilies=1), raises=dict(mpl="ValueError", seaborn="ValueError")),
}
EXCEPTIONS = {"ValueError": ValueError, "LinAlgError": np.linalg.LinAlgError}


def raises_of(name, method):
    return CASES[name].get("raises", {}).get(method)


def _lengths(n, salt, lo, span):
    with np.errstate(over="ignore"):
        return lo + (splitmix64(np.arange(n, dtype=U) + U(salt)) % U(span)).astype(np.float64)


def build_case(name):
    """{matrix name: DataFrame, or DataFrame.to_json() string for the "run" case}: what distribution() is handed, matrix by matrix."""
    case = CASES[name]
    kind = case["kind"]
    if kind == "equal":
        return {"m": pd.DataFrame(np.full((case["n"], case["n"]), 1.0))}
    I, C = family_matrices(**case["gen"])
    n = len(I)
    if kind == "run":      # the five matrices of a run as the Run row stores them (integer genome ids from 1)
        from pyani_amd.anim import run_matrices_to_json
        ids = list(range(1, n + 1))
        aln = np.floor(C * _lengths(n, 977, 800000.0, 200000)[:, None])
        mats = {"identity": I, "coverage": C, "aln_lengths": aln, "sim_errors": np.floor((1.0 - I) * aln), "hadamard": I * C}
        return run_matrices_to_json({k: pd.DataFrame(v, index=ids, columns=ids) for k, v in mats.items()})
    if kind == "coverage":      # exact zeros: pairs without any alignment
        with np.errstate(over="ignore"):
            h = splitmix64(np.arange(n * n, dtype=U) + (U(case["gen"]["seed"]) << U(44))).reshape(n, n)
        C[h % U(7) == U(0)] = 0.0
        return {"m": pd.DataFrame(C)}
    if kind in ("aln_lengths", "sim_errors"):      # values up to 10^7; sim_errors as the integer frame read_json makes of it
        aln = np.floor(C * _lengths(n, 1977, 2000000.0, 8000000)[:, None])
        if kind == "aln_lengths":
            return {"m": pd.DataFrame(aln)}
        return {"m": pd.DataFrame(np.floor((1.0 - I) * aln).astype(np.int64))}
    for e in case.get("edits", ()):
        if e == "clip":      # every pair within a sub-family ends exactly on the top edge
            I = np.minimum(I + 0.03, 1.0)
        elif e == "round2":
            I = np.round(I, 2)
        elif e == "nan":
            I[3, 7] = np.nan
    return {"m": pd.DataFrame(I)}


def as_frame(f):
    """A case's frame the way the reference receives it (write_run_plots reads the stored strings with pd.read_json)."""
    import io
    return pd.read_json(io.StringIO(f)) if isinstance(f, str) else f


def flat(f):
    """The values distribution() works on: dfr.values.flatten(), as float64."""
    return np.ascontiguousarray(as_frame(f).values.flatten(), dtype=np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def density_tolerance(n, ref):
    """The bound on |density - ref|.  scipy's value is a sequential sum of n non-negative terms: worst-case relative error n * 2^-53
    (a blocked sum is tighter).  A rounding of the exponent's argument is amplified by the exponent's magnitude a, and terms with
    a > 745 underflow to 0: at most about 2^-40.  Derived, not tuned."""
    return (n * 2.0 ** -53 + 2.0 ** -40) * np.abs(np.asarray(ref, dtype=np.float64)) + 1e-300


def density_close(got, ref, n):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and bool(np.all(np.abs(got - ref) <= density_tolerance(n, ref)))


def max_rel_error(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = ref > 0
    return float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0


# ---- the bandwidth: the reference's number is not one number ---------------------------------------------------------------------
# gaussian_kde's data covariance is np.cov's dot product, which numpy hands to its BLAS.  A BLAS splits a long dot product over its
# threads, so scipy's OWN bandwidth changes in the last bits with the thread count and the machine: for the 10^6 values of
# n1000_clipped, on one host, 0.003267566878793516 / ...5015 / ...498 / ...499 with 1 / 2 / 4 / 8 BLAS threads, and ...4976 on another
# host with 16.  A recorded value can therefore be met bit for bit only where it was recorded.  What the contract says ("scipy's
# number, not a differently summed one") is checked as it can be on every machine: bit for bit against scipy's estimator run in the
# same process on the same values, and that live value against the recorded one within the rounding bound of an n-term sum.
def live_reference_bandwidth(x):
    """(cho_cov[0, 0], sqrt(covariance)) of scipy.stats.gaussian_kde(x) as distribution() builds it, computed here and now."""
    from scipy.stats import gaussian_kde
    kde = gaussian_kde(x)
    kde._compute_covariance()
    return float(kde.cho_cov[0, 0]), float(np.sqrt(kde.covariance.squeeze()))


def bandwidth_tolerance(n, ref):
    """Two orderings of the covariance's n-term sum of non-negative products differ by at most n * 2^-53 relative (the centring sum
    adds the same order again); the square root halves it.  2 n * 2^-53 covers both sums."""
    return 2.0 * n * 2.0 ** -53 * abs(float(ref))


def check_against_gold(name, method, mat, arrays, x, got):
    """The asserts shared by the CPU test, the GPU test and the probe.  x: the case's flat values.  Counts and bin edges: the golden's,
    exactly.  Bandwidth: scipy's live value bit for bit, and within bandwidth_tolerance of the golden's.  Support: "mpl" the golden's
    bits (it does not depend on the bandwidth); "seaborn" the bits of the grid seaborn's rule makes of the live bandwidth, and within
    3 bandwidth tolerances of the golden's.  Density: within density_tolerance of scipy's stored value and of the high-precision one."""
    edges, counts, support, density, bw = got
    key = f"{mat}|{method}"
    used = x[~np.isnan(x)]
    n = used.size
    assert same_bits(edges, arrays[f"{key}|edges"]), f"{name} {key}: bin edges"
    assert counts.dtype == np.int64 and np.array_equal(counts, arrays[f"{key}|counts"]), f"{name} {key}: counts"
    gold_bw = float(arrays[f"{key}|bandwidth"][0])
    live_bw, live_grid_bw = live_reference_bandwidth(used)
    print(f"{name} {key}: bandwidth {bw!r}, scipy here {live_bw!r}, golden {gold_bw!r}")
    assert same_bits(bw, live_bw), f"{name} {key}: bandwidth differs from scipy's on the same values in this process"
    assert abs(live_bw - gold_bw) <= bandwidth_tolerance(n, gold_bw), f"{name} {key}: scipy's bandwidth here against the golden"
    gold_support = arrays[f"{key}|support"]
    if method == "mpl":
        assert same_bits(support, gold_support), f"{name} {key}: support"
    else:
        lo, hi = float(used.min()), float(used.max())
        assert same_bits(support, np.linspace(lo - live_grid_bw * CUT, hi + live_grid_bw * CUT, GRID)), f"{name} {key}: support"
        slack = CUT * bandwidth_tolerance(n, gold_bw) + 4 * np.finfo(np.float64).eps * np.abs(gold_support)
        assert support.shape == gold_support.shape and np.all(np.abs(support - gold_support) <= slack), f"{name} {key}: support against the golden"
    for ref in ("density", "density_hp"):
        print(f"{name} {key}: max relative difference to {ref} {max_rel_error(density, arrays[f'{key}|{ref}']):.3g}")
        assert density_close(density, arrays[f"{key}|{ref}"], n), f"{name} {key}: density against {ref}"


# ---- golden files: one .npz per case -------------------------------------------------------------------------------------------
def load_gold(name):
    """(meta, arrays): meta is the JSON record; arrays the npz members "<matrix>|<method>|<edges / counts / support / density /
    density_hp / bandwidth>" (float64 bits kept; counts int64; density_hp: the high-precision density T)."""
    with np.load(GOLDEN_DIR / f"{name}.npz", allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(str(z["meta"]))
    return meta, arrays


# ---- the independent restatement -----------------------------------------------------------------------------------------------
def restate_counts(x, edges):
    """np.histogram's rule by sorting: bin i holds the values with edges[i] <= x < edges[i + 1], the last bin its right edge too; NaN
    and values outside are not counted."""
    x = np.sort(x[~np.isnan(x)])
    at = np.searchsorted(x, edges, side="left")
    at[-1] = np.searchsorted(x, edges[-1], side="right")
    return np.diff(at).astype(np.int64)


def restate_bandwidth(x):
    """(cho_cov[0, 0], sqrt(covariance)) of gaussian_kde(x): scipy's own sequence of numpy calls, restated from its source."""
    n = x.size
    if n <= 1:
        raise ValueError("`dataset` input should have multiple elements.")
    w = np.ones(n) / n
    factor = np.power(1 / np.sum(w ** 2), -1.0 / (1 + 4))
    c = np.atleast_2d(np.cov(x.reshape(1, n), rowvar=1, bias=False, aweights=w))
    if not np.isfinite(c).all():
        raise ValueError("array must not contain infs or NaNs")
    if c[0, 0] <= 0:
        raise np.linalg.LinAlgError("singular data covariance")
    return float((np.sqrt(c) * factor)[0, 0]), float(np.sqrt((c * factor ** 2).squeeze()))


def restate_density(x, support, bw, block=4096):
    """gaussian_kde(x)(support): per-block numpy sums of exp(-((p - x) / bw)^2 / 2), the blocks added in order, then scipy's
    normalisation (weights 1 / n, (2 pi)^(-1/2) / bw)."""
    s = np.zeros(len(support), dtype=np.float64)
    for k in range(0, len(x), block):
        t = (support[:, None] - x[None, k:k + block]) / bw
        s += np.exp(-(t * t) / 2.0).sum(axis=1)
    return s * (np.power(2 * np.pi, -0.5) / bw) / len(x)


def restate(x, method):
    """(edges, counts, support, density, bandwidth) of the flat float64 values x, or raises what the reference raises."""
    x = np.asarray(x, dtype=np.float64)
    if method == "mpl":
        if not np.isfinite(x).all():
            raise ValueError("array must not contain infs or NaNs")
    else:
        x = x[~np.isnan(x)]
    bw, grid_bw = restate_bandwidth(x)
    lo, hi = float(x.min()), float(x.max())
    if method == "mpl":
        a, b = (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)
        edges = np.linspace(a, b, BINS + 1)
        support = np.linspace(lo, hi, GRID)
    else:
        edges = np.histogram_bin_edges(x, "auto", (lo, hi))
        support = np.linspace(lo - grid_bw * CUT, hi + grid_bw * CUT, GRID)
    return edges, restate_counts(x, edges), support, restate_density(x, support, bw), bw


class HostEngine:
    """Stands in for the device in the CPU test of the product's host pieces: the three device results from numpy, and a record of
    what was asked."""

    def __init__(self):
        self.loads = self.releases = 0
        self.x = None

    def dist_load(self, x):
        self.loads += 1
        self.x = np.asarray(x, dtype=np.float64).reshape(-1)
        ok = self.x[~np.isnan(self.x)]
        return (float(ok.min()) if ok.size else np.inf, float(ok.max()) if ok.size else -np.inf, int(np.isnan(self.x).sum()),
                int(np.isinf(self.x).sum()))

    def dist_hist(self, edges):
        assert self.x is not None
        return restate_counts(self.x, np.asarray(edges, dtype=np.float64))

    def dist_kde(self, points, bandwidth):
        assert self.x is not None
        x = self.x[~np.isnan(self.x)]
        return restate_density(x, np.asarray(points, dtype=np.float64), bandwidth) * len(x) / (np.power(2 * np.pi, -0.5) / bandwidth)

    def dist_release(self):
        self.releases += 1
        self.x = None
