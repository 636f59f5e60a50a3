#!/usr/bin/env python3
"""Measure the distribution plots' arithmetic on the GPU: n = 1000 / 2000 / 4000 / 8192 genomes (n x n values), a single matrix and
the five matrices of a run.

Before anything is timed the n = 1000 golden (tests/golden/distribution: n1000_clipped, both methods) is checked: counts, edges,
support and bandwidth as the tests check them (tests/distribution_cases.py: check_against_gold), the density within the tests' bound.  Then, per size, on an asymmetric identity-like matrix of
tests/classify_cases.family_matrices, medians of --repeats runs after one warm-up:

  stats / hist / kde_kernel_ms   pg_dist_last_ms: HIP events round the kernels of pg_dist_load, pg_dist_hist (50 bins) and pg_dist_kde
                                 (200 points), and the density kernel's fp64 exponentials per second (n^2 * 200 / time)
  upload_seconds                 pg_dist_load's wall time less its kernel time: the copy of 8 n^2 bytes from pageable memory
  host_bandwidth_seconds         the host's numpy pass for scipy's Scott bandwidth (graphics.scott_bandwidth)
  distribution_data_seconds      pyani_amd.graphics.distribution_data end to end, method="mpl"
  run_distributions_seconds      five matrices of a run
  density_max_rel_error_vs_scipy where scipy is timed

scipy's gaussian_kde (construction and evaluation on the 200-point grid) and np.histogram(bins=50) are timed once in the same run on
the same host, one core, up to --scipy-up-to genomes.  Writes profiles/distribution_probe.json.

Usage: python tools/distribution_probe.py [--repeats 5] [--sizes 1000,2000,4000,8192] [--scipy-up-to 4000] [--out ...]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402
import pandas as pd     # noqa: E402

from pyani_amd import _lib, graphics      # noqa: E402
from pyani_amd.engine import Engine       # noqa: E402
from tests import distribution_cases as dc      # noqa: E402
from tests.classify_cases import family_matrices      # noqa: E402


def check_golden(eng):
    name = "n1000_clipped"
    meta, arrays = dc.load_gold(name)
    f = dc.build_case(name)["m"]
    for method in dc.METHODS:
        dc.check_against_gold(name, method, "m", arrays, dc.flat(f), graphics.distribution_data(f, method=method, engine=eng))
    return [name]


def median_of(repeats, fn):
    fn()      # warm-up
    vals = [fn() for _ in range(repeats)]
    return statistics.median(vals), vals


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1000,2000,4000,8192")
    ap.add_argument("--scipy-up-to", type=int, default=4000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "distribution_probe.json"))
    args = ap.parse_args()
    try:
        import scipy
        from scipy.stats import gaussian_kde
        baseline = {"source": f"scipy {scipy.__version__} and numpy {np.__version__}, timed once per size in this run on this host, one core"}
    except ImportError:
        gaussian_kde = None
        baseline = {"source": "scipy not importable here: no baseline was timed"}
    report = {"library": _lib.load().pg_version().decode(), "repeats": args.repeats, "baseline": baseline, "sizes": {}}
    with Engine(0) as eng:
        report["goldens_checked_first"] = check_golden(eng)
        print("golden ok:", report["goldens_checked_first"], flush=True)
        for n in [int(s) for s in args.sizes.split(",")]:
            I, C = family_matrices(n=n, seed=80 + n % 7, families=10, subfamilies=4, asym=30000)
            x = np.ascontiguousarray(I).reshape(-1)
            rec = {"n": n, "values": int(x.size)}
            eng.profile_enable(True)      # kernel times only; the end-to-end figures below are taken with it off
            lo, hi, _, _ = eng.dist_load(x)
            edges, support = np.linspace(lo, hi, graphics.DIST_BINS + 1), np.linspace(lo, hi, graphics.DIST_GRID)
            bw = graphics.scott_bandwidth(x)[0]

            def load_times():
                wall = timed(lambda: eng.dist_load(x))
                return wall, eng.dist_last_ms()[0]

            load_times()
            loads = [load_times() for _ in range(args.repeats)]
            rec["stats_kernel_ms"] = round(statistics.median(k for _, k in loads), 4)
            rec["upload_seconds"] = round(statistics.median(w - k * 1e-3 for w, k in loads), 5)
            med, vals = median_of(args.repeats, lambda: (eng.dist_hist(edges), eng.dist_last_ms()[1])[1])
            rec["hist_kernel_ms"], rec["hist_kernel_ms_all"] = round(med, 4), [round(v, 4) for v in vals]
            med, vals = median_of(args.repeats, lambda: (eng.dist_kde(support, bw), eng.dist_last_ms()[2])[1])
            rec["kde_kernel_ms"], rec["kde_kernel_ms_all"] = round(med, 4), [round(v, 4) for v in vals]
            rec["kde_fp64_exponentials_per_second"] = round(x.size * float(len(support)) / (med * 1e-3), 0)
            eng.profile_enable(False)
            med, vals = median_of(args.repeats, lambda: timed(lambda: graphics.scott_bandwidth(x)))
            rec["host_bandwidth_seconds"] = round(med, 5)
            frame = pd.DataFrame(I)
            med, vals = median_of(args.repeats, lambda: timed(lambda: graphics.distribution_data(frame, engine=eng)))
            rec["distribution_data_seconds"], rec["distribution_data_seconds_all"] = round(med, 5), [round(v, 5) for v in vals]
            run = {"identity": frame, "coverage": pd.DataFrame(C), "aln_lengths": pd.DataFrame(np.floor(C * 1e6)),
                   "sim_errors": pd.DataFrame(np.floor((1.0 - I) * 1e4)), "hadamard": pd.DataFrame(I * C)}
            med, vals = median_of(args.repeats, lambda: timed(lambda: graphics.run_distributions(run, engine=eng)))
            rec["run_distributions_seconds"], rec["run_distributions_seconds_all"] = round(med, 5), [round(v, 5) for v in vals]
            if gaussian_kde is not None and n <= args.scipy_up_to:
                got = graphics.distribution_data(frame, engine=eng)
                t0 = time.perf_counter()
                kde = gaussian_kde(x)
                kde._compute_covariance()
                ref = kde(got.support)
                t1 = time.perf_counter()
                counts = np.histogram(x, bins=graphics.DIST_BINS)[0]
                t2 = time.perf_counter()
                assert np.array_equal(counts, got.counts) and dc.same_bits(kde.cho_cov[0, 0], got.bandwidth)
                assert dc.density_close(got.density, ref, x.size)
                rec["scipy_seconds"] = {"gaussian_kde": round(t1 - t0, 4), "np_histogram": round(t2 - t1, 5)}
                rec["density_max_rel_error_vs_scipy"] = dc.max_rel_error(got.density, ref)
            report["sizes"][str(n)] = rec
            print(n, json.dumps(rec), flush=True)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
