#!/usr/bin/env python3
"""Measure neighbour joining on the GPU: n = 100 / 1000 / 2000 / 4000 / 8192 nodes of an identity-like distance matrix.

Per size, medians of --repeats runs after one warm-up:

  call_seconds        Engine.tree_nj end to end (upload of the matrix, validation, every step, read-back)
  validate_ms / wide_ms / tail_ms   the stage milliseconds of pg_tree_nj_last (HIP events, profiling on, a run of its own)
  statement_seconds   pyani_amd.tree.nj_of_matrix on the host, one run, up to --statement-up-to nodes; the device's result is checked
                      for equality with it (integers equal, doubles bit for bit) wherever it ran

and, at --tail-size nodes, a table of whole-call seconds over tail_limit (3 = every step wide ... 1024), every run checked against the
default's result.  Writes profiles/tree_probe.json.

Usage: python tools/tree_probe.py [--repeats 3] [--sizes 100,1000,2000,4000,8192] [--statement-up-to 2000] [--out profiles/tree_probe.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402

from pyani_amd import _lib, tree      # noqa: E402
from pyani_amd.engine import Engine   # noqa: E402

TAIL_LIMITS = (3, 64, 128, 256, 512, 768, 1024)


def matrix(n):
    """1 - identity for identities 0.70 ... 1.00 given to four decimals."""
    ident = np.round(np.random.default_rng(n).uniform(0.70, 1.0, (n, n)), 4)
    upper = np.triu(1.0 - ident, 1)
    return upper + upper.T


def same(a, b):
    return all(x.tobytes() == np.asarray(y, dtype=x.dtype).tobytes() for x, y in zip(a, b))


def median_of(repeats, fn):
    fn()      # warm-up
    vals = [fn() for _ in range(repeats)]
    return statistics.median(vals), vals


def timed_call(eng, d):
    t0 = time.perf_counter()
    eng.tree_nj(d)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="100,1000,2000,4000,8192")
    ap.add_argument("--statement-up-to", type=int, default=2000)
    ap.add_argument("--tail-size", type=int, default=2000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tree_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "repeats": args.repeats, "sizes": {}, "tail_limit": {}}
    with Engine(0) as eng:
        for n in [int(s) for s in args.sizes.split(",")]:
            d = matrix(n)
            rec = {"n": n}
            got = eng.tree_nj(d)
            if n <= args.statement_up_to:
                t0 = time.perf_counter()
                want = tree.nj_of_matrix(d)
                rec["statement_seconds"] = round(time.perf_counter() - t0, 4)
                assert same(got, (want.joins, want.lengths, want.last, want.last_lengths)), f"n = {n}: the device differs from the statement"
                rec["equal_to_statement"] = True
            med, vals = median_of(args.repeats, lambda: timed_call(eng, d))
            rec["call_seconds"], rec["call_seconds_all"] = round(med, 5), [round(v, 5) for v in vals]
            if "statement_seconds" in rec:
                rec["statement_over_call"] = round(rec["statement_seconds"] / med, 2)
            eng.profile_enable(True)
            try:
                stages = []
                for _ in range(args.repeats + 1):
                    assert same(eng.tree_nj(d), got)
                    stages.append(eng.tree_nj_last()[1])
            finally:
                eng.profile_enable(False)
            for key in stages[0]:
                rec[key] = round(statistics.median(s[key] for s in stages[1:]), 4)
            rec["counts"] = eng.tree_nj_last()[0]
            report["sizes"][str(n)] = rec
            print(n, json.dumps(rec), flush=True)
        d = matrix(args.tail_size)
        base = eng.tree_nj(d)
        table = {}
        for tail in TAIL_LIMITS:
            eng.tree_nj_set(tail)
            assert same(eng.tree_nj(d), base), f"tail_limit {tail}: the result changed"
            med, vals = median_of(args.repeats, lambda: timed_call(eng, d))
            table[str(tail)] = {"call_seconds": round(med, 5), "call_seconds_all": [round(v, 5) for v in vals]}
            print("tail_limit", tail, table[str(tail)], flush=True)
        eng.tree_nj_set(512)
        report["tail_limit"] = {"n": args.tail_size, "table": table}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
