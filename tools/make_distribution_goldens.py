#!/usr/bin/env python3
"""Generate tests/golden/distribution/*.npz for the cases of tests/distribution_cases.py.

Runs only where the reference tree exists (a checkout beside this repository, or $PYANI_REFERENCE) together with scipy and
matplotlib.  method="mpl": the reference's OWN pyani_graphics.mpl.distribution is run (Agg backend); bar heights are read from
axes[0].patches, the curve from axes[1].lines[0]; the patches' sides are the bin edges only up to the rounding of hist()'s bar
placement, so the edges' bits are numpy's answer to the call hist() makes, checked against the sides; its module imports without seaborn once `pyani.pyani_graphics` is entered in
sys.modules as an empty package.  The bandwidth is gaussian_kde(data).cho_cov[0, 0] after _compute_covariance(), as distribution()
calls it; that estimator's curve must equal the drawn one bit for bit or the tool stops.  method="seaborn": seaborn is not available,
so that leg makes the numpy / scipy calls seaborn's histplot and kdeplot make with their defaults (NaN dropped;
np.histogram_bin_edges(x, "auto", (min, max)); gaussian_kde(x), set_bandwidth(factor); grid np.linspace(min - 3 bw, max + 3 bw, 200)
with bw = sqrt(covariance); np.histogram) — numpy's and scipy's answers, not a run of seaborn; the metadata says so.

Per case and method a high-precision density T is stored too: numpy longdouble terms summed with math.fsum.  scipy's own value must
meet the tests' bound (tests/distribution_cases.py: density_tolerance) against T, and the test-only restatement must reproduce edges,
counts, support and bandwidth exactly and the density within the bound; a case that fails is reported and NOT written (the bound is
not widened).  DATA only — no reference source text is written anywhere.

Usage: python tools/make_distribution_goldens.py [case ...]"""
import json
import math
import os
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("PYANI_REFERENCE", ROOT.parent / "reference"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "bio_shim"))
sys.path.insert(0, str(REF))

import matplotlib      # noqa: E402
matplotlib.use("Agg")
import matplotlib.pyplot as plt      # noqa: E402
import numpy as np                   # noqa: E402
import pandas as pd                  # noqa: E402
import scipy                         # noqa: E402
from scipy.stats import gaussian_kde      # noqa: E402

from tests import distribution_cases as dc      # noqa: E402


def load_reference():
    pkg = types.ModuleType("pyani.pyani_graphics")
    pkg.__path__ = [str(REF / "pyani" / "pyani_graphics")]
    sys.modules["pyani.pyani_graphics"] = pkg
    import pyani.pyani_graphics.mpl as ref_mpl
    return ref_mpl


def high_precision_density(x, support, bw):
    """T: every term in longdouble, each point's terms summed with math.fsum, scipy's normalisation in longdouble."""
    L = np.longdouble
    xs, h = x.astype(L), L(bw)
    norm = L(1) / (np.sqrt(L(2) * L(np.pi)) * h)      # pi to double precision: 6e-17 relative
    out = np.empty(len(support), dtype=np.float64)
    for j, p in enumerate(support):
        t = (L(p) - xs) / h
        out[j] = float(L(math.fsum(np.exp(-(t * t) / L(2)).tolist())) * norm / L(len(x)))
    return out


def reference_mpl(ref_mpl, frame, matname):
    """(edges, counts, support, density) as the reference's own distribution() drew them."""
    fig = ref_mpl.distribution(frame, None, matname)
    try:
        patches = fig.axes[0].patches
        left = np.array([p.get_x() for p in patches], dtype=np.float64)
        right = np.array([p.get_x() + p.get_width() for p in patches], dtype=np.float64)
        counts = np.array([p.get_height() for p in patches], dtype=np.float64)
        line = fig.axes[1].lines[0]
        return left, right, counts, np.asarray(line.get_xdata(), dtype=np.float64), np.asarray(line.get_ydata(), dtype=np.float64)
    finally:
        plt.close(fig)


def leg_mpl(ref_mpl, frame, matname):
    left, right, heights, support, density = reference_mpl(ref_mpl, frame, matname)
    data = frame.values.flatten()
    counts, edges = np.histogram(data, bins=dc.BINS, range=(np.nanmin(data), np.nanmax(data)))      # what Axes.hist asks numpy for
    # hist() draws bar i centred on edges[i] + width / 2 with that width, so a patch's sides are the edges after two roundings: the
    # heights are read from the figure, the edges' bits from numpy's answer to hist()'s own call, checked against the patches' sides
    slack = 4 * np.finfo(np.float64).eps * max(abs(edges[0]), abs(edges[-1]), edges[-1] - edges[0])
    assert len(left) == dc.BINS and np.array_equal(heights, counts)
    assert np.abs(left - edges[:-1]).max() <= slack and np.abs(right - edges[1:]).max() <= slack
    kde = gaussian_kde(data)
    kde._compute_covariance()
    if not dc.same_bits(kde(support), density):
        raise SystemExit("the drawn curve is not gaussian_kde(data)(xvals)")
    return edges, counts.astype(np.int64), support, density, float(kde.cho_cov[0, 0])


def leg_seaborn(frame):
    x = frame.values.flatten().astype(np.float64)
    x = x[~np.isnan(x)]
    kde = gaussian_kde(x)
    kde.set_bandwidth(kde.factor * 1)
    bw = np.sqrt(kde.covariance.squeeze())
    support = np.linspace(x.min() - bw * dc.CUT, x.max() + bw * dc.CUT, dc.GRID)
    edges = np.histogram_bin_edges(x, "auto", (x.min(), x.max()))
    counts = np.histogram(x, edges)[0]
    return edges, counts.astype(np.int64), support, kde(support), float(kde.cho_cov[0, 0])


def run_case(name, ref_mpl):
    meta = {"case": name, "matrices": {}, "scipy": scipy.__version__, "numpy": np.__version__, "pandas": pd.__version__,
            "matplotlib": matplotlib.__version__,
            "provenance": {"mpl": "bars and curve read from the figure of the reference's own pyani_graphics.mpl.distribution; the "
                                  "bandwidth from the scipy estimator it builds",
                           "seaborn": "numpy's and scipy's answers to the calls seaborn's histplot and kdeplot make with their defaults; "
                                      "seaborn was not available, so this is not the reference's own run"}}
    arrays = {}
    for mat, f in dc.build_case(name).items():
        frame = dc.as_frame(f)
        x = dc.flat(f)
        rec = {"n": int(x.size)}
        for method in dc.METHODS:
            key = f"{mat}|{method}"
            try:
                edges, counts, support, density, bw = leg_mpl(ref_mpl, frame, mat) if method == "mpl" else leg_seaborn(frame)
            except (ValueError, np.linalg.LinAlgError) as err:
                rec[method] = {"raises": type(err).__name__, "message": str(err)[:200]}
                assert dc.raises_of(name, method) == type(err).__name__, (name, method, type(err).__name__)
                try:
                    dc.restate(x, method)
                except dc.EXCEPTIONS[type(err).__name__]:
                    continue
                raise SystemExit(f"{name} {key}: the restatement does not raise {type(err).__name__}")
            assert dc.raises_of(name, method) is None, (name, method)
            used = x[~np.isnan(x)]
            T = high_precision_density(used, support, bw)
            if not dc.density_close(density, T, used.size):
                print(f"{name} {key}: scipy's own density misses the bound against T (max rel {dc.max_rel_error(density, T):.3g}): case NOT written")
                return None, None
            r_edges, r_counts, r_support, r_density, r_bw = dc.restate(x, method)
            if not (dc.same_bits(r_edges, edges) and np.array_equal(r_counts, counts) and dc.same_bits(r_support, support)
                    and dc.same_bits(r_bw, bw)):
                raise SystemExit(f"{name} {key}: the restated edges / counts / support / bandwidth differ from the reference's")
            if not (dc.density_close(r_density, density, used.size) and dc.density_close(r_density, T, used.size)):
                raise SystemExit(f"{name} {key}: the restated density misses the bound")
            rec[method] = {"raises": None, "n_used": int(used.size), "bins": int(len(counts)),
                           "scipy_vs_T_max_rel": dc.max_rel_error(density, T)}
            arrays[f"{key}|edges"], arrays[f"{key}|counts"], arrays[f"{key}|support"] = edges, counts, support
            arrays[f"{key}|density"], arrays[f"{key}|density_hp"], arrays[f"{key}|bandwidth"] = density, T, np.array([bw], dtype=np.float64)
        meta["matrices"][mat] = rec
    return meta, arrays


def main(names):
    ref_mpl = load_reference()
    dc.GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
    for name in names or list(dc.CASES):
        meta, arrays = run_case(name, ref_mpl)
        if meta is None:
            continue
        path = dc.GOLDEN_DIR / f"{name}.npz"
        np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
        print(f"{name}: arrays={len(arrays)} -> {path.stat().st_size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
