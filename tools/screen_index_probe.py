#!/usr/bin/env python3
"""Measure the screen's index path on one MI355X: against the dense path where both exist, alone beyond it.

  both paths   C4 (bench.py's ANIm set: 1000 genomes of ~5 Mb, scale 256) and a synthetic set of 8192 genomes (pyani_amd.synth families
               of 25, --length bases each, scale --scale): Engine.screen_candidates at identity 0.80 with path="dense" and path="index"
               on the same resident genomes — wall milliseconds of the whole call (best of --repeats after one warm-up), the stage
               milliseconds of pg_screen_last / pg_screen_index_last of the last run, whether the two ScreenedPairs are equal, and
               index_over_dense = index wall / dense wall.
  index alone  n = 16 384 and 32 768 of the same synthetic families: wall and stage milliseconds, kept pairs, index bytes
               (4 E + 8 (G + 1)), bands and band rows.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_index_probe.json.

Usage: python tools/screen_index_probe.py [--sets C4,8192,16384,32768] [--length 20000] [--scale 16] [--repeats 3]
                                          [--out profiles/screen_index_probe.json]"""
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


def load(eng, seed, n_generator, n, length):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(seed, n_generator, g, length), range(n)))
    ids = [eng.add_genome(s, o) for s, o in data]
    bases = sum(len(s) for s, _ in data)
    del data
    eng.upload()
    return ids, bases, round(time.perf_counter() - t0, 2)


def run(eng, ids, opt, path, repeats):
    """(ScreenedPairs, wall milliseconds of every run after the warm-up, the stage record of the last run)."""
    eng.screen_candidates(ids, opt, path=path)      # warm-up: code objects, allocations
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sp = eng.screen_candidates(ids, opt, path=path)
        walls.append((time.perf_counter() - t0) * 1e3)
    last = eng.screen_last() if path == "dense" else eng.screen_index_last()
    return sp, walls, last


def record(path, sp, walls, last):
    rec = {"wall_ms_best": round(min(walls), 3), "wall_ms_all": [round(w, 3) for w in walls], "kept_pairs": int(len(sp.a)),
           "stages": {k: (round(v, 3) if k.endswith("_ms") else v) for k, v in last.items()}}
    if path == "index":
        rec["index_bytes"] = 4 * last["entries"] + 8 * (last["groups"] + 1)
        rec["bands"] = last["bands"]
        rec["band_rows"] = screen.default_band_rows(len(sp.sizes))
    return rec


def probe(eng, name, args):
    eng.clear_genomes()
    if name == "C4":
        cfg = synth.SETS["C4"]
        n, scale = cfg["n"], 256
        ids, bases, prep = load(eng, cfg["seed"], cfg["n"], n, cfg["L"])
    else:
        n, scale = int(name), args.scale
        ids, bases, prep = load(eng, SEED, n, n, args.length)
    opt = screen.ScreenOptions(THRESHOLD, KMER, scale)
    rec = {"set": name, "genomes": n, "bases": bases, "prepare_seconds": prep, "options": dict(opt._asdict()), "ordered_pairs": n * (n - 1)}
    print(name, "resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)
    index, walls, last = run(eng, ids, opt, "index", args.repeats)
    rec["index"] = record("index", index, walls, last)
    if n <= screen.DENSE_MAX_GENOMES:
        dense, walls, last = run(eng, ids, opt, "dense", args.repeats)
        rec["dense"] = record("dense", dense, walls, last)
        rec["equal"] = bool((index.sizes == dense.sizes).all() and all((getattr(index, f) == getattr(dense, f)).all() for f in ("a", "b", "shared")))
        rec["index_over_dense"] = round(rec["index"]["wall_ms_best"] / rec["dense"]["wall_ms_best"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C4,8192,16384,32768")
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_index_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "synthetic_length": args.length, "sets": []}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with Engine(0) as eng:
        for name in (x for x in args.sets.split(",") if x):
            report["sets"].append(probe(eng, name, args))
            print(json.dumps(report["sets"][-1]), flush=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
