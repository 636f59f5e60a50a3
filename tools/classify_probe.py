#!/usr/bin/env python3
"""Measure the classify stage on the GPU for the two large golden cases (1000 genomes: bit matrix in LDS; 1500: in device memory).

Per case and per memberships mode ("none", "special", "all"): wall time of pyani_amd.classify.classify() end to end (median of
--repeats runs after one warm-up) and the two profile slots of pg_profile_get (edge kernel; death + sweep kernels) from one profiled
run — beside the reference's wall time recorded in the golden (one CPU core, networkx) and the time of the test-only host restatement
(tests/classify_cases.py: sort + serial union-find, one core) on the same input.  The answers are checked against the golden before
anything is timed.  Writes profiles/classify_probe.json.

Usage: python tools/classify_probe.py [--repeats 5] [--out profiles/classify_probe.json]"""
import argparse
import gzip
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_amd import _lib, classify      # noqa: E402
from pyani_amd.engine import Engine      # noqa: E402
from tests import classify_cases as cc      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "classify_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "repeats": args.repeats, "cases": {}}
    with Engine(0) as eng:
        for name in ("n1000_default", "n1500_default"):
            with gzip.open(ROOT / "tests" / "golden" / "classify" / f"{name}.json.gz", "rt") as fh:
                gold = json.load(fh)
            par = gold["params"]
            I, C, labels = cc.build_case(name)
            seq = classify.classify(I, C, labels, memberships="none", engine=eng, **par)
            got = [[float(s.interval), *s.cliqueinfo] for s in seq]
            assert got == [[float(t[0]), *t[1:]] for t in gold["tuples"]], f"{name}: the GPU sequence differs from the golden"
            rec = {"n": gold["n"], "edges": gold["n_edges"], "steps": len(seq), "resolution": par["resolution"],
                   "sweep_path": "LDS" if gold["n"] <= 1024 else "device memory",
                   "reference_seconds": gold["reference_seconds"], "gpu": {}}
            for mode in ("none", "special", "all"):
                walls = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    classify.classify(I, C, labels, memberships=mode, engine=eng, **par)
                    walls.append(time.perf_counter() - t0)
                eng.profile_enable(True)
                eng.profile_config()
                eng.profile_reset()
                classify.classify(I, C, labels, memberships=mode, engine=eng, **par)
                edge, sweep = eng.profile_get(_lib.K_CLASSIFY_EDGE), eng.profile_get(_lib.K_CLASSIFY_SWEEP)
                eng.profile_enable(False)
                eng.profile_reset()
                rec["gpu"][mode] = {"wall_seconds_median": round(statistics.median(walls), 5), "wall_seconds_all": [round(w, 5) for w in walls],
                                    "edge_kernel_ms": round(edge[0], 4), "edge_launches": edge[1],
                                    "death_and_sweep_kernels_ms": round(sweep[0], 4), "sweep_calls": sweep[1]}
            host = {}
            for mode, parts in (("none", False), ("all", True)):
                t0 = time.perf_counter()
                cc.restate(I, C, partitions=parts, **par)
                host[mode] = round(time.perf_counter() - t0, 4)
            rec["host_restatement_seconds"] = host
            report["cases"][name] = rec
            print(name, json.dumps(rec), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
