#!/usr/bin/env python3
"""Measure the two mappings of the sketch mode side by side — "anywhere" (pg_sketch_pairs_k) and "window" (pg_sketch_pairs_mapped) — on
the workload of tools/sketch_k_probe.py: 200 synthetic genomes of 5 Mb from the bench generator, all 39 800 ordered pairs, k = 16, 14
and 12, frag_len 3000, scale 16, in ONE process.

Per k and mapping, after a warm-up call on two small extra genomes (loads the kernels, builds nothing of the set):

  build_seconds              the first call over the n self pairs: "anywhere" builds every genome's sketch; "window" (run second, the
                             sketches resident) builds every genome's position index and grouped sketch and maps the n self pairs;
                             index_build_ms is pg_sketch_map_last_ms' build part of that call (HIP events)
  pairs_per_second           all ordered pairs with everything resident, median of --repeats calls (every call ends in a synchronise);
                             map_kernel_ms: pg_sketch_map_last_ms' kernel part of the last "window" call
  related / unrelated share  of the pairs that get a result (status 0); related = same ancestor of the generator
  vs_exact                   mean and maximum |sketch ANI - anim_pairs identity| in the identity tiers >= 0.90, 0.80 ... 0.90, < 0.80 over
                             the fixed sample of --exact-pairs related pairs tools/sketch_k_probe.py uses
  window_over_anywhere       ratio of the two pairs_per_second

Writes profiles/sketch_map_probe.json.
Usage: python tools/sketch_map_probe.py [--n 200] [--L 5000000] [--ks 16,14,12] [--repeats 3] [--exact-pairs 600] [--out ...]"""
import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def leg(eng, ids, warm, q, r, k, mapping, repeats):
    kw = {"kmer": k, "mapping": mapping}
    eng.sketch_pairs([warm[0]], [warm[1]], **kw)      # warm-up: this k's kernels on two small genomes
    t_build, _ = timed(lambda: eng.sketch_pairs(ids, ids, **kw))
    rec = {"build_seconds": t_build}
    if mapping == "window":
        rec["index_build_ms"] = eng.sketch_map_last_ms()[0]
    runs = [timed(lambda: eng.sketch_pairs(q, r, **kw)) for _ in range(repeats)]
    secs = [t for t, _ in runs]
    rec.update({"pairs": int(len(q)), "pairs_seconds_all": secs, "pairs_per_second": len(q) / statistics.median(secs)})
    if mapping == "window":
        rec["map_kernel_ms"] = eng.sketch_map_last_ms()[1]
    return rec, runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=20250228)
    ap.add_argument("--ks", default="16,14,12")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--exact-pairs", type=int, default=600)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sketch_map_probe.json"))
    args = ap.parse_args()
    from pyani_amd import _lib, synth
    from pyani_amd.engine import Engine

    n, L = args.n, args.L
    K = (n + 24) // 25      # the generator's ancestors: genome g descends from ancestor g % K
    with ThreadPoolExecutor(16) as pool:
        data = list(pool.map(lambda g: synth.genome(args.seed, n, g, L), range(n)))
    small = [synth.genome(args.seed + 1, 2, g, 100_000) for g in range(2)]
    out = Path(args.out)
    with Engine(0) as eng:
        ids = np.array([eng.add_genome(s, o) for s, o in data], dtype=np.int32)
        warm = [eng.add_genome(s, o) for s, o in small]
        del data
        eng.upload()
        a, b = np.divmod(np.arange(n * n), n)
        keep = a != b
        q, r = ids[a[keep]], ids[b[keep]]
        related = (a[keep] % K) == (b[keep] % K)
        report = {"library": _lib.load().pg_version().decode(), "repeats": args.repeats,
                  "workload": f"{n} synthetic genomes of {L} bp (bench generator, seed {args.seed}, {K} ancestors), all {int(keep.sum())} ordered pairs, "
                              "frag_len 3000, scale 16, min_fraction 0.2; both mappings in one process"}
        pick = np.flatnonzero(related)
        pick = pick[:: max(1, len(pick) // max(1, args.exact_pairs))][: args.exact_pairs]
        t_exact, exact = timed(lambda: eng.anim_pairs(r[pick], q[pick]))      # nucmer's query = the sketch's query
        ok = exact["status"] == 0
        ident = exact["identity"]
        report["exact_sample"] = {"pairs": int(len(pick)), "anim_pairs_seconds": t_exact, "with_alignment": int(ok.sum())}
        report["k"] = {}
        for k in [int(x) for x in args.ks.split(",")]:
            report["k"][str(k)] = {}
            for mapping in ("anywhere", "window"):
                rec, res = leg(eng, ids, warm, q, r, k, mapping, args.repeats)
                got = res["status"] == 0
                rec["related_pairs"], rec["unrelated_pairs"] = int(related.sum()), int((~related).sum())
                rec["related_share_with_result"] = float((got & related).sum() / max(1, related.sum()))
                rec["unrelated_share_with_result"] = float((got & ~related).sum() / max(1, (~related).sum()))
                rec["unrelated_matches_max"] = int(res["matches"][~related].max()) if (~related).any() else 0
                both = ok & got[pick]
                err = np.abs(res["ani"][pick] - ident)
                tiers = {}
                for name, sel in (("identity_ge_0.90", ident >= 0.90), ("identity_0.80_to_0.90", (ident >= 0.80) & (ident < 0.90)), ("identity_lt_0.80", ident < 0.80)):
                    m = both & sel
                    tiers[name] = {"pairs": int(m.sum()), "mean_abs_error": float(err[m].mean()) if m.any() else None, "max_abs_error": float(err[m].max()) if m.any() else None}
                rec["vs_exact"] = tiers
                report["k"][str(k)][mapping] = rec
                print(k, mapping, json.dumps(rec), flush=True)
            report["k"][str(k)]["window_over_anywhere"] = report["k"][str(k)]["window"]["pairs_per_second"] / report["k"][str(k)]["anywhere"]["pairs_per_second"]
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
