#!/usr/bin/env python3
"""Measure the search index on disk and its shrinking on one MI355X.

  set       the synthetic collection of tools/screen_search_probe.py: 32 768 + 1024 genomes (pyani_amd.synth, families of 25, --length
            bases each, scale --scale), every 33rd held out, the first 64 of those the queries.
  measured  best of --repeats after one warm-up, wall milliseconds of the whole Python call.  Every configuration's search result is
            asserted equal to the one-shot index's (the kept triples of Engine.screen_search at identity 0.80) BEFORE its time is
            recorded.
              save     Engine.screen_search_index_save: the export and the file; the file's bytes
              load     Engine.screen_search_index_load: the read (np.memmap), the upload, the validation on the device (its HIP-event
                       milliseconds apart) and the sizes' comparison
              drivers  run_screen_search over the FASTA files of the collection against run_screen_search(index=) on the same queries
                       (--fasta 0 leaves this out: it writes the whole collection as FASTA files into a temporary directory)
              remove   Engine.screen_search_index_remove of 64, 1024 and half the columns (chosen by a seeded generator), each against
                       Engine.screen_search_index over the survivors in the same run; the stages of pg_screen_search_remove_last and the
                       compaction's achieved bytes per second, counting the arrays it streams: 12 E read (member, pos), 4 E' written,
                       20 D read (kmer, start, gpos), 12 D' written — the gathers of new_of and of pos at the starts are not counted.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_search_store_probe.json.

Usage: python tools/screen_search_store_probe.py [--genomes 32768] [--length 20000] [--scale 16] [--repeats 3] [--fasta 1]
                                                 [--out profiles/screen_search_store_probe.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np      # noqa: E402

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402
from pyani_amd.subcmd_search import run_screen_search      # noqa: E402
from pyani_amd.subcmd_searchdb import run_screen_index_build      # noqa: E402
from screen_search_probe import KMER, SEED, THRESHOLD, load, rounded      # noqa: E402


def timed(fn, repeats, before=None):
    """Best of `repeats` after one warm-up; before(): untimed, ahead of every run (a destructive call gets its state back)."""
    walls, out = [], None
    for i in range(repeats + 1):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
    return out, {"wall_ms_best": round(min(walls), 3), "wall_ms_all": [round(w, 3) for w in walls]}


def triples(hits):
    return hits.a.copy(), hits.b.copy(), hits.shared.copy()


def same(x, y):
    return all(len(a) == len(b) and (a == b).all() for a, b in zip(x, y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fasta", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_search_store_probe.json"))
    args = ap.parse_args()
    scale, n = args.scale, args.genomes + args.genomes // 32
    opt = screen.ScreenOptions(THRESHOLD, KMER, scale)
    rep = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "scale": scale, "min_identity": THRESHOLD, "synthetic_length": args.length,
           "repeats": args.repeats}
    with Engine(0) as eng, tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        ids, bases, prep = load(eng, SEED, n, n, args.length)
        held = [g for g in range(n) if g % 33 == 32]
        held_set = set(held)
        db = [g for g in range(n) if g not in held_set]
        queries = held[:64]
        db_ids, q_ids = [ids[g] for g in db], [ids[g] for g in queries]
        labels = [f"g{g:06d}" for g in db]
        rep.update(db_genomes=len(db), queries=len(queries), bases=bases, prepare_seconds=prep)
        print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)

        # the one-shot index: every configuration below is held to its result
        _, rep["index"] = timed(lambda: eng.screen_search_index(db_ids, KMER, scale, labels=labels), args.repeats)
        built = eng.screen_search_last()
        rep["index"]["stages"] = rounded({k: built[k] for k in ("keys", "kmers", "entries", "slices", "index_bytes", "index_scan_ms", "index_sort_group_ms")})
        want = triples(eng.screen_search(q_ids, opt))

        path = tmp / "probe.idx"
        size, rep["save"] = timed(lambda: eng.screen_search_index_save(path), args.repeats)
        rep["save"]["file_bytes"] = int(size)
        rep["save"]["GB_per_s"] = round(size / rep["save"]["wall_ms_best"] / 1e6, 3)
        validation = []

        def load_file():
            out = eng.screen_search_index_load(path)
            validation.append(eng.screen_search_last()["index_sort_group_ms"])
            return out
        eng.screen_search_index_release()
        _, rec = timed(load_file, args.repeats, before=eng.screen_search_index_release)
        assert same(triples(eng.screen_search(q_ids, opt)), want), "the loaded index searches differently"
        loaded = eng.screen_search_last()
        assert all(loaded[k] == built[k] for k in ("keys", "kmers", "entries", "slices"))
        rec["file_bytes"] = int(size)
        rec["GB_per_s"] = round(size / rec["wall_ms_best"] / 1e6, 3)
        rec["validation_ms_best"] = round(min(validation[1:]), 3)
        rec["validation_GB_per_s"] = round((12 * loaded["kmers"] + 4 * loaded["entries"]) / min(validation[1:]) / 1e6, 3)
        rec["index_bytes"] = loaded["index_bytes"]
        rep["load"] = rec
        print("save", rep["save"], "load", rep["load"], flush=True)

        # remove against a rebuild over the survivors, in the same run
        rng = np.random.default_rng(SEED)
        rep["remove"] = []
        for m in (64, 1024, len(db) // 2):
            cols = np.sort(rng.choice(len(db), size=m, replace=False))
            keep = np.ones(len(db), dtype=bool)
            keep[cols] = False
            left_ids = [db_ids[i] for i in np.flatnonzero(keep)]
            _, rebuild = timed(lambda: eng.screen_search_index(left_ids, KMER, scale), args.repeats)
            fresh, fresh_last = triples(eng.screen_search(q_ids, opt)), eng.screen_search_last()
            _, removed = timed(lambda: eng.screen_search_index_remove(cols.tolist()), args.repeats,
                               before=lambda: eng.screen_search_index(db_ids, KMER, scale))
            assert same(triples(eng.screen_search(q_ids, opt)), fresh), f"the index without {m} genomes searches differently"
            last, rem = eng.screen_search_last(), eng.screen_search_remove_last()
            assert (last["kmers"], last["entries"]) == (fresh_last["kmers"], fresh_last["entries"])
            moved = 12 * built["entries"] + 4 * last["entries"] + 20 * built["kmers"] + 12 * last["kmers"]
            rec = {"removed_genomes": m, "remove": removed, "rebuild_over_survivors": rebuild, "stages": rounded(rem), "kmers_after": last["kmers"],
                   "entries_after": last["entries"], "compaction_bytes": moved,
                   "compaction_GB_per_s": round(moved / rem["compact_ms"] / 1e6, 3) if rem["compact_ms"] else None,
                   "rebuild_over_remove": round(rebuild["wall_ms_best"] / removed["wall_ms_best"], 3)}
            rep["remove"].append(rec)
            print(json.dumps(rec), flush=True)
        eng.screen_search_index_release()

        # the drivers: the collection read as FASTA files against the saved index
        if args.fasta:
            db_dir, q_dir = tmp / "db", tmp / "queries"
            db_dir.mkdir()
            q_dir.mkdir()
            t0 = time.perf_counter()
            jobs = [(db_dir, name, g) for g, name in zip(db, labels)] + [(q_dir, f"q{g:06d}", g) for g in queries]
            with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
                list(ex.map(lambda j: synth.write_fasta(j[0] / f"{j[1]}.fna", *synth.genome(SEED, n, j[2], args.length), j[1]), jobs))
            eng.clear_genomes()
            rec = {"fasta_write_seconds": round(time.perf_counter() - t0, 2)}
            t0 = time.perf_counter()
            made = run_screen_index_build(db_dir, tmp / "built.idx", kmer=KMER, scale=scale, engine=eng)
            rec["index_build_seconds"] = round(time.perf_counter() - t0, 2)
            rec["file_bytes"] = made.file_bytes
            a, rec["from_fasta"] = timed(lambda: run_screen_search(db_dir, q_dir, min_identity=THRESHOLD, kmer=KMER, scale=scale, engine=eng), args.repeats)
            b, rec["from_index"] = timed(lambda: run_screen_search(None, q_dir, min_identity=THRESHOLD, kmer=KMER, scale=scale, engine=eng,
                                                                   index=tmp / "built.idx"), args.repeats)
            assert a.frame.equals(b.frame) and same(triples(a.hits), triples(b.hits)) and len(a.hits.a) == len(want[0]), "the drivers disagree"
            rec["kept"] = int(len(a.hits.a))
            rec["fasta_over_index"] = round(rec["from_fasta"]["wall_ms_best"] / rec["from_index"]["wall_ms_best"], 3)
            rep["drivers"] = rec
            print(json.dumps(rec), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rep, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
