#!/usr/bin/env python3
"""Measure the screen's search on one MI355X against the only route there was before it.

  sets      "32768+64" and "32768+1024": the synthetic families of tools/screen_index_probe.py (pyani_amd.synth, families of 25, --length
            bases each, scale --scale), 32 768 + 1024 genomes generated, every 33rd held out as a query (so every query has relatives
            in the collection) — all 1024 of them, or the first 64.  "C4+16": bench.py's ANIm set (1000 genomes of ~5 Mb, scale 256),
            every 62nd held out, 16 queries against 984.
  measured  per set, best of --repeats after one warm-up, wall milliseconds of the whole Python call and the HIP events of
            pg_screen_search_last of the last run:
              index    Engine.screen_search_index(db)
              search   Engine.screen_search(queries) at identity 0.80 against the resident index
              parent   Engine.screen_candidates(db + queries, path="index") and the host filter of the query rows x db columns
            whether search and parent give the same triples, parent / search, and each stage's share of the search's device time.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_search_probe.json.

Usage: python tools/screen_search_probe.py [--sets 32768+64,32768+1024,C4+16] [--length 20000] [--scale 16] [--repeats 3]
                                           [--out profiles/screen_search_probe.json]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402

KMER, THRESHOLD, SEED = 16, 0.80, 20261908
STAGES = ("scan_ms", "sort_group_ms", "lookup_ms", "count_ms", "select_ms")


def load(eng, seed, n_generator, n, length):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(seed, n_generator, g, length), range(n)))
    ids = [eng.add_genome(s, o) for s, o in data]
    bases = sum(len(s) for s, _ in data)
    del data
    eng.upload()
    return ids, bases, round(time.perf_counter() - t0, 2)


def timed(fn, repeats):
    fn()      # warm-up: code objects, allocations
    walls, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, {"wall_ms_best": round(min(walls), 3), "wall_ms_all": [round(w, 3) for w in walls]}


def rounded(last):
    return {k: (round(v, 3) if k.endswith("_ms") else v) for k, v in last.items()}


def probe(eng, name, args):
    eng.clear_genomes()
    base, n_q = name.split("+")
    n_q = int(n_q)
    if base == "C4":
        cfg = synth.SETS["C4"]
        n, scale, stride = cfg["n"], 256, cfg["n"] // n_q
        ids, bases, prep = load(eng, cfg["seed"], cfg["n"], n, cfg["L"])
        held = [g for g in range(n) if g % stride == stride - 1][:n_q]
    else:
        n, scale = int(base) + 1024, args.scale
        ids, bases, prep = load(eng, SEED, n, n, args.length)
        held = [g for g in range(n) if g % 33 == 32]      # 1024 of 33 792: the collection is the other 32 768, whatever n_q
    held_set = set(held)
    db = [g for g in range(n) if g not in held_set]
    queries = held[:n_q]
    db_ids, q_ids = [ids[g] for g in db], [ids[g] for g in queries]
    opt = screen.ScreenOptions(THRESHOLD, KMER, scale)
    rec = {"set": name, "db_genomes": len(db), "queries": len(queries), "bases": bases, "prepare_seconds": prep, "options": dict(opt._asdict())}
    print(name, "resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)

    _, rec["index"] = timed(lambda: eng.screen_search_index(db_ids, KMER, scale), args.repeats)
    built = eng.screen_search_last()
    rec["index"]["stages"] = rounded({k: built[k] for k in ("keys", "kmers", "entries", "slices", "index_scan_ms", "index_sort_group_ms")})
    rec["index"]["index_bytes_held"] = built["index_bytes"]      # the allocated sizes of the resident buffers (pg_screen_search_last)
    rec["index"]["index_bytes_used"] = 12 * (built["kmers"] + 1) + 4 * built["entries"]      # computed: 12 (D + 1) + 4 E

    hits, rec["search"] = timed(lambda: eng.screen_search(q_ids, opt), args.repeats)
    last = eng.screen_search_last()      # (of the last chunk: one chunk at these sizes)
    rec["search"]["chunks"] = -(-len(q_ids) // screen.default_search_rows(len(db_ids)))
    rec["search"]["kept"] = int(len(hits.a))
    rec["search"]["stages"] = rounded({k: last[k] for k in ("query_keys", "lookups", "matched", "increments", "query_slices") + STAGES})
    device = sum(last[k] for k in STAGES)
    rec["search"]["stage_share"] = {k: round(last[k] / device, 4) if device else None for k in STAGES}
    eng.screen_search_index_release()

    def parent():
        sp = eng.screen_candidates(db_ids + q_ids, opt, path="index")
        rows = (sp.a >= len(db_ids)) & (sp.b < len(db_ids))
        return sp.a[rows] - np.int32(len(db_ids)), sp.b[rows], sp.shared[rows]
    old, rec["parent"] = timed(parent, args.repeats)
    rec["parent"]["stages"] = rounded(eng.screen_index_last())
    rec["equal"] = bool(all(len(x) == len(y) and (x == y).all() for x, y in zip(old, (hits.a, hits.b, hits.shared))))
    rec["parent_over_search"] = round(rec["parent"]["wall_ms_best"] / rec["search"]["wall_ms_best"], 3)
    rec["parent_over_index_plus_search"] = round(rec["parent"]["wall_ms_best"] / (rec["index"]["wall_ms_best"] + rec["search"]["wall_ms_best"]), 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="32768+64,32768+1024,C4+16")
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_search_probe.json"))
    args = ap.parse_args()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "synthetic_length": args.length, "sets": []}
    if out.exists():      # sets measured by an earlier call stay: a set is replaced by its new record
        report["sets"] = [s for s in json.loads(out.read_text()).get("sets", []) if s.get("set") not in args.sets.split(",")]
    with Engine(0) as eng:
        for name in (x for x in args.sets.split(",") if x):
            report["sets"].append(probe(eng, name, args))
            print(json.dumps(report["sets"][-1]), flush=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
