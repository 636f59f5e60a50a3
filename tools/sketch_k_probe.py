#!/usr/bin/env python3
"""Measure the sketch mode (pg_sketch_pairs_k) at k = 16, 14 and 12 on the C2-size synthetic set: 200 genomes of 5 Mb from the bench
generator, all 39 800 ordered pairs, frag_len 3000, scale 16.

Per k, after a warm-up call on two small extra genomes (loads that k's kernels, builds nothing of the set):

  sketch_build_seconds       one call over the n self pairs: builds every genome's sketch (scan kernel, twice per genome)
  pairs_per_second           all ordered pairs with the sketches resident, median of --repeats calls (every call ends in a synchronise)
  related / unrelated share  of the pairs that get a result (status 0); related = same ancestor of the generator
  vs_exact                   mean and maximum |sketch ANI - anim_pairs identity| in the identity tiers of tests/test_sketch_gpu.py
                             (>= 0.90, 0.80 ... 0.90, < 0.80) over a fixed sample of --exact-pairs related pairs

The k = 16 leg calls eng.sketch_pairs(q, r) with DEFAULTS only, so `--k16-only` runs unchanged on a commit without the kmer keyword:
that is how the default path is compared with the parent commit (`--series-into` appends the leg's figures to a named series of the
output file).  Writes profiles/sketch_k_probe.json.

Usage: python tools/sketch_k_probe.py [--n 200] [--L 5000000] [--ks 16,14,12] [--repeats 3] [--exact-pairs 600] [--out ...]
       python tools/sketch_k_probe.py --k16-only --series-into parent|this [--out ...]"""
import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

import numpy as np      # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def leg(eng, ids, warm, q, r, k, repeats):
    """Build seconds, pairs per second and the records of one k; k = 16 goes through the defaults."""
    kw = {} if k == 16 else {"kmer": k}
    eng.sketch_pairs([warm[0]], [warm[1]], **kw)      # warm-up: this k's kernels, two small sketches
    t_build, _ = timed(lambda: eng.sketch_pairs(ids, ids, **kw))
    runs = [timed(lambda: eng.sketch_pairs(q, r, **kw)) for _ in range(repeats)]
    secs = [t for t, _ in runs]
    return {"sketch_build_seconds": t_build, "pairs": int(len(q)), "pairs_seconds_all": secs,
            "pairs_per_second": len(q) / statistics.median(secs)}, runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=20250228)
    ap.add_argument("--ks", default="16,14,12")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--exact-pairs", type=int, default=600)
    ap.add_argument("--k16-only", action="store_true")
    ap.add_argument("--series-into", default=None, help="append the k = 16 leg's figures to report['default_path'][NAME]")
    ap.add_argument("--package-root", default=str(ROOT), help="the tree whose pyani_amd is measured")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sketch_k_probe.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    from pyani_amd import _lib, synth
    from pyani_amd.engine import Engine

    n, L = args.n, args.L
    K = (n + 24) // 25      # the generator's ancestors: genome g descends from ancestor g % K
    with ThreadPoolExecutor(16) as pool:
        data = list(pool.map(lambda g: synth.genome(args.seed, n, g, L), range(n)))
    small = [synth.genome(args.seed + 1, 2, g, 100_000) for g in range(2)]
    out = Path(args.out)
    report = json.loads(out.read_text()) if out.exists() else {}
    with Engine(0) as eng:
        ids = np.array([eng.add_genome(s, o) for s, o in data], dtype=np.int32)
        warm = [eng.add_genome(s, o) for s, o in small]
        del data
        eng.upload()
        a, b = np.divmod(np.arange(n * n), n)
        keep = a != b
        q, r = ids[a[keep]], ids[b[keep]]
        related = (a[keep] % K) == (b[keep] % K)
        if args.k16_only:
            rec, _ = leg(eng, ids, warm, q, r, 16, args.repeats)
            print(json.dumps(rec), flush=True)
            if args.series_into:
                series = report.setdefault("default_path", {}).setdefault(args.series_into, {"library": _lib.load().pg_version().decode(), "sketch_build_seconds": [], "pairs_per_second": []})
                series["sketch_build_seconds"].append(rec["sketch_build_seconds"])
                series["pairs_per_second"].append(rec["pairs_per_second"])
                out.parent.mkdir(parents=True, exist_ok=True)
                out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
            return
        report.update({"library": _lib.load().pg_version().decode(), "repeats": args.repeats,
                       "workload": f"{n} synthetic genomes of {L} bp (bench generator, seed {args.seed}, {K} ancestors), all {int(keep.sum())} ordered pairs, "
                                   "frag_len 3000, scale 16, min_fraction 0.2"})
        # the exact engine on a fixed sample of the related pairs: nucmer's query = the sketch's query
        pick = np.flatnonzero(related)
        pick = pick[:: max(1, len(pick) // max(1, args.exact_pairs))][: args.exact_pairs]
        t_exact, exact = timed(lambda: eng.anim_pairs(r[pick], q[pick]))
        ok = exact["status"] == 0
        ident = exact["identity"]
        report["exact_sample"] = {"pairs": int(len(pick)), "anim_pairs_seconds": t_exact, "with_alignment": int(ok.sum())}
        report["k"] = {}
        for k in [int(x) for x in args.ks.split(",")]:
            rec, res = leg(eng, ids, warm, q, r, k, args.repeats)
            got = res["status"] == 0
            rec["related_pairs"], rec["unrelated_pairs"] = int(related.sum()), int((~related).sum())
            rec["related_share_with_result"] = float((got & related).sum() / max(1, related.sum()))
            rec["unrelated_share_with_result"] = float((got & ~related).sum() / max(1, (~related).sum()))
            both = ok & got[pick]
            err = np.abs(res["ani"][pick] - ident)
            tiers = {}
            for name, sel in (("identity_ge_0.90", ident >= 0.90), ("identity_0.80_to_0.90", (ident >= 0.80) & (ident < 0.90)), ("identity_lt_0.80", ident < 0.80)):
                m = both & sel
                tiers[name] = {"pairs": int(m.sum()), "mean_abs_error": float(err[m].mean()) if m.any() else None, "max_abs_error": float(err[m].max()) if m.any() else None}
            rec["vs_exact"] = tiers
            report["k"][str(k)] = rec
            print(k, json.dumps(rec), flush=True)
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
