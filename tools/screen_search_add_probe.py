#!/usr/bin/env python3
"""Measure the growth of the search index on one MI355X against the only route there was before it: the rebuild.

  set       the synthetic collection of tools/screen_search_probe.py: 32 768 + 1024 genomes (pyani_amd.synth, families of 25, --length
            bases each, scale --scale), every 33rd held out; the collection is the other 32 768, the queries the first 64 held out.
  (a) add   for m = 64 and m = 1024: Engine.screen_search_index(the first 32 768 - m) [not timed], then
            Engine.screen_search_index_add(the last m) [timed], against Engine.screen_search_index(all 32 768) in the same run — the
            existing call, the yardstick.  Wall milliseconds of the Python call, best of --repeats after one warm-up, and the HIP events
            of pg_screen_search_add_last; D, E, new and matched k-mers; the device bytes of the two indexes that exist side by side
            while the add runs, and the add's work arrays by the formula of pyani_gpu.h.
  (b) batch the whole index built in batches of --batch genomes through a store cleared after every batch (load, index or add, clear),
            against the one-shot build: the milliseconds inside the index / add calls, summed, and the wall time with the loading.
  (c) equal every configuration's Engine.screen_search over the 64 queries must equal the one-shot index's, triple for triple, BEFORE
            its time is recorded: a configuration that differs aborts the probe.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_search_add_probe.json.

Usage: python tools/screen_search_add_probe.py [--length 20000] [--scale 16] [--repeats 3] [--batch 4096]
                                               [--out profiles/screen_search_add_probe.json]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402

KMER, THRESHOLD, SEED = 16, 0.80, 20261908
N_DB, N_HELD, N_QUERIES = 32768, 1024, 64
ADD_STAGES = ("scan_ms", "sort_group_ms", "merge_ms")


def rounded(last):
    return {k: (round(v, 3) if k.endswith("_ms") else v) for k, v in last.items()}


def best(walls):
    return {"wall_ms_best": round(min(walls), 3), "wall_ms_all": [round(w, 3) for w in walls]}


def ms_of(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def same(hits, ref, what):
    for x, y in zip((hits.a, hits.b, hits.shared, hits.db_sizes), (ref.a, ref.b, ref.shared, ref.db_sizes)):
        if len(x) != len(y) or not (x == y).all():
            raise SystemExit(f"{what}: the search over the grown index differs from the one-shot index's")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_search_add_probe.json"))
    args = ap.parse_args()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    n = N_DB + N_HELD
    opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "scale": args.scale, "min_identity": THRESHOLD, "synthetic_length": args.length,
              "db_genomes": N_DB, "queries": N_QUERIES, "repeats": args.repeats}
    t0 = time.perf_counter()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(SEED, n, g, args.length), range(n)))
    held = [g for g in range(n) if g % 33 == 32]
    held_set = set(held)
    db, queries = [g for g in range(n) if g not in held_set], held[:N_QUERIES]
    report["generate_seconds"] = round(time.perf_counter() - t0, 2)

    with Engine(0) as eng:
        ids = [eng.add_genome(*data[g]) for g in range(n)]
        eng.upload()
        db_ids, q_ids = [ids[g] for g in db], [ids[g] for g in queries]

        # the yardstick: the one-shot build, and its search result
        eng.screen_search_index(db_ids, KMER, args.scale)      # warm-up
        walls = [ms_of(lambda: eng.screen_search_index(db_ids, KMER, args.scale)) for _ in range(args.repeats)]
        built = eng.screen_search_last()
        ref = eng.screen_search(q_ids, opt)
        report["rebuild"] = dict(best(walls), stages=rounded({k: built[k] for k in ("keys", "kmers", "entries", "slices", "index_scan_ms", "index_sort_group_ms")}),
                                 index_bytes=built["index_bytes"], kept=int(len(ref.a)))
        print("rebuild", json.dumps(report["rebuild"]), flush=True)

        # (a) one add against one rebuild
        report["add"] = []
        for m in (64, 1024):
            base, tail = db_ids[:N_DB - m], db_ids[N_DB - m:]
            walls, rec = [], {"m": m}
            for rep in range(args.repeats + 1):      # the first is the warm-up
                eng.screen_search_index(base, KMER, args.scale)
                base_last = eng.screen_search_last()
                w = ms_of(lambda: eng.screen_search_index_add(tail))
                add, merged = eng.screen_search_add_last(), eng.screen_search_last()
                rec["equal"] = same(eng.screen_search(q_ids, opt), ref, f"add of {m}")      # (c): before the time counts
                if rep:
                    walls.append(w)
            rec.update(best(walls))
            rec["stages"] = rounded(add)
            device = sum(add[k] for k in ADD_STAGES)
            rec["stage_share"] = {k: round(add[k] / device, 4) if device else None for k in ADD_STAGES}
            rec["base"] = {k: base_last[k] for k in ("kmers", "entries", "slices", "index_bytes")}
            rec["merged"] = {k: merged[k] for k in ("keys", "kmers", "entries", "slices", "index_bytes")}
            assert (merged["kmers"], merged["entries"]) == (built["kmers"], built["entries"])
            rec["both_indexes_bytes"] = base_last["index_bytes"] + merged["index_bytes"]
            rec["work_arrays_bytes"] = 38 * add["entries"] + 4 * (base_last["kmers"] + 1)      # staged twice, runs, ranks, flags | ins
            rec["add_over_rebuild"] = round(rec["wall_ms_best"] / report["rebuild"]["wall_ms_best"], 4)
            report["add"].append(rec)
            print("add", json.dumps(rec), flush=True)
        eng.screen_search_index_release()

        # (b) the whole index in batches through a cleared store
        calls, totals, n_batches = [], [], 0
        for rep in range(args.repeats + 1):
            eng.clear_genomes()
            t0 = time.perf_counter()
            inside, n_batches = 0.0, 0
            for lo in range(0, N_DB, args.batch):
                part = [eng.add_genome(*data[g]) for g in db[lo:lo + args.batch]]
                eng.upload()
                inside += ms_of((lambda: eng.screen_search_index(part, KMER, args.scale)) if lo == 0 else (lambda: eng.screen_search_index_add(part)))
                eng.clear_genomes()
                n_batches += 1
            total = (time.perf_counter() - t0) * 1e3
            grown = eng.screen_search_last()
            assert (grown["kmers"], grown["entries"], grown["keys"]) == (built["kmers"], built["entries"], built["keys"])
            same(eng.screen_search([eng.add_genome(*data[g]) for g in queries], opt), ref, "batches")      # (c)
            if rep:
                calls.append(inside)
                totals.append(total)
        report["batches"] = {"batch": args.batch, "batches": n_batches, "equal": True, "index_and_add_calls": best(calls), "with_loading": best(totals),
                             "last_add": rounded(eng.screen_search_add_last()), "index_bytes": grown["index_bytes"],
                             "calls_over_rebuild": round(min(calls) / report["rebuild"]["wall_ms_best"], 3)}
        print("batches", json.dumps(report["batches"]), flush=True)
        eng.screen_search_index_release()
        eng.clear_genomes()
    out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
