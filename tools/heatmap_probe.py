#!/usr/bin/env python3
"""Measure the heatmap clustering on the GPU: n = 1000 / 2000 / 4000 / 8192 genomes, a single matrix and a run's ten-problem batch.

Before anything is timed the answers are checked against the goldens (tests/golden/heatmap: n1000, n2000, n3072; distances by
SHA-1, Z bit for bit, both orientations and both methods).  Then, per size, on an asymmetric identity-like matrix of
tests/classify_cases.family_matrices, medians of --repeats runs after one warm-up:

  pdist_kernel_ms        the profile slot of cluster_pdist_kernel for one orientation (rows), and its fp64 operations per second
                         counted as 3 n (n - 1) / 2 m (subtract, multiply, add per pair and element; the square roots are not counted)
  linkage_kernel_ms      the profile slot of cluster_linkage_kernel, one problem ("complete" and "average")
  heatmap_order_seconds  pyani_amd.graphics.heatmap_order end to end (upload, two clusterings, host sort / relabel / leaves, frame)
  batch10                run_heatmap_orders on five matrices (ten problems): wall, and the two slots summed over the batch

If scipy can be imported its pdist and linkage are timed on the same inputs in the same run (one core, up to --scipy-up-to
observations); if not, the figures measured on a different machine are quoted and labelled so.  Writes profiles/heatmap_probe.json.

Usage: python tools/heatmap_probe.py [--repeats 5] [--sizes 1000,2000,4000,8192] [--out profiles/heatmap_probe.json]"""
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
from tests import heatmap_cases as hc     # noqa: E402
from tests.classify_cases import family_matrices      # noqa: E402


def check_goldens(eng):
    checked = []
    for name in ("n1000", "n2000", "n3072"):
        meta, arrays = hc.load_gold(name)
        frame = hc.build_case(name)[0]["m"].sort_index()
        x = np.ascontiguousarray(frame.to_numpy(dtype=np.float64))
        for o in hc.ORIENTATIONS:
            d = eng.cluster_pdist(x, columns=(o == "col"))
            assert hc.sha1(d) == meta["matrices"]["m"][o]["dist_sha1"], f"{name} {o}: distances differ from the golden"
            for method in hc.METHODS:
                Z = graphics.linkage(x, method=method, columns=(o == "col"), engine=eng)
                assert hc.same_bits(Z, hc.gold_z(arrays, f"m|{o}", method)), f"{name} {o} {method}: Z differs from the golden"
        checked.append(name)
    return checked


def slots(eng, fn):
    eng.profile_enable(True)
    eng.profile_config()
    eng.profile_reset()
    try:
        fn()
        return eng.profile_get(_lib.K_CLUSTER_PDIST), eng.profile_get(_lib.K_CLUSTER_LINKAGE)
    finally:
        eng.profile_enable(False)
        eng.profile_reset()


def median_of(repeats, fn):
    fn()      # warm-up
    vals = [fn() for _ in range(repeats)]
    return statistics.median(vals), vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1000,2000,4000,8192")
    ap.add_argument("--scipy-up-to", type=int, default=2000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "heatmap_probe.json"))
    args = ap.parse_args()
    try:
        import scipy
        import scipy.cluster.hierarchy as sch
        from scipy.spatial import distance
        baseline = {"source": f"scipy {scipy.__version__}, timed in this run on this host, one core"}
    except ImportError:
        sch = distance = None
        baseline = {"source": "scipy not importable here; measured on a DIFFERENT machine (the build host), one core",
                    "pdist_seconds": {"1000": 0.26, "2000": 1.94}, "linkage_seconds": {"2000": 0.07}}
    report = {"library": _lib.load().pg_version().decode(), "repeats": args.repeats, "baseline": baseline, "sizes": {}}
    with Engine(0) as eng:
        report["goldens_checked_first"] = check_goldens(eng)
        print("goldens ok:", report["goldens_checked_first"], flush=True)
        for n in [int(s) for s in args.sizes.split(",")]:
            I, C = family_matrices(n=n, seed=70 + n % 7, families=10, subfamilies=4, asym=30000)
            frame = pd.DataFrame(I)
            rec = {"n": n}

            def pdist_ms():
                return slots(eng, lambda: eng.cluster_pdist(I))[0][0]

            med, vals = median_of(args.repeats, pdist_ms)
            ops = 3.0 * n * (n - 1) / 2.0 * n
            rec["pdist_kernel_ms"] = round(med, 4)
            rec["pdist_kernel_ms_all"] = [round(v, 4) for v in vals]
            rec["pdist_fp64_ops_per_second"] = round(ops / (med * 1e-3), 0)
            for method in hc.METHODS:
                code = graphics.METHODS[method]
                med, vals = median_of(args.repeats, lambda: slots(eng, lambda: eng.cluster_linkage(I, method=code))[1][0])
                rec[f"linkage_kernel_ms_{method}"] = round(med, 4)
                rec[f"linkage_kernel_ms_{method}_all"] = [round(v, 4) for v in vals]

            def order_seconds():
                t0 = time.perf_counter()
                graphics.heatmap_order(frame, engine=eng)
                return time.perf_counter() - t0

            med, vals = median_of(args.repeats, order_seconds)
            rec["heatmap_order_seconds"] = round(med, 5)
            rec["heatmap_order_seconds_all"] = [round(v, 5) for v in vals]
            run = {"identity": frame, "coverage": pd.DataFrame(C), "aln_lengths": pd.DataFrame(np.floor(C * 1e6)),
                   "sim_errors": pd.DataFrame(np.floor((1.0 - I) * 1e4)), "hadamard": pd.DataFrame(I * C)}

            def batch_seconds():
                t0 = time.perf_counter()
                graphics.run_heatmap_orders(run, engine=eng)
                return time.perf_counter() - t0

            med, vals = median_of(args.repeats, batch_seconds)
            (p_ms, p_n), (l_ms, l_n) = slots(eng, lambda: graphics.run_heatmap_orders(run, engine=eng))
            rec["batch10"] = {"wall_seconds": round(med, 5), "wall_seconds_all": [round(v, 5) for v in vals],
                              "pdist_kernels_ms_sum": round(p_ms, 4), "pdist_launches": p_n,
                              "linkage_kernel_ms": round(l_ms, 4), "linkage_launches": l_n}
            if sch is not None and n <= args.scipy_up_to:
                t0 = time.perf_counter()
                d = distance.pdist(I)
                t1 = time.perf_counter()
                sch.linkage(d, method="complete")
                t2 = time.perf_counter()
                rec["scipy_seconds"] = {"pdist": round(t1 - t0, 4), "linkage_complete": round(t2 - t1, 4)}
                assert hc.same_bits(d, eng.cluster_pdist(I))
            report["sizes"][str(n)] = rec
            print(n, json.dumps(rec), flush=True)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
