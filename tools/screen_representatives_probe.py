#!/usr/bin/env python3
"""Measure the greedy representatives of the screen's kept pairs on one MI355X.  Every timed call runs --repeats times
after one warm-up; the MEDIAN wall milliseconds of the whole Python call are reported beside every run's, and the HIP-event
milliseconds and counts of pg_screen_representatives_last of the last run.

  index entry  Engine.screen_dereplicate(path="index") on the 32 768-genome synthetic set of tools/screen_index_probe.py at identity
               0.80 — the index built, all bands selected, the undirected kept pairs appended on the device, ranks, rounds, assign — and
               its stages from a run of its own; the bytes read back.
  host         the way to the same table without the kernels: Engine.screen_candidates(path="index") + the host statement
               screen.representatives_of_pairs; the bytes read back.
  list entry   Engine.screen_representatives on the kept pairs of that set (both directions, as the selection returns them).
  components   Engine.screen_components_of(path="index") on the same set, for comparison: the single-linkage answer.
  random       a list of 2^20 nodes and --entries entries (10^8), random 40-bit scores.
  chain        4096 nodes, scores falling along it: 2048 rounds, the bad case.

Live-entry compaction between batches was NOT tried: the rounds read the whole list every time.  No time is set in advance: what is
measured is recorded, and what is not is listed under "not_measured".  Writes profiles/screen_representatives_probe.json.

Usage: python tools/screen_representatives_probe.py [--genomes 32768] [--length 20000] [--scale 16] [--entries 100000000] [--repeats 3]
                                                    [--out profiles/screen_representatives_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402

KMER, THRESHOLD, SEED = 16, 0.80, 20261908      # tools/screen_index_probe.py's: the same synthetic families of 25
MAX_N = 1 << 20
STAGES = ("select_ms", "sort_ms", "rounds_ms", "assign_ms")


def load(eng, seed, n, length):
    t0 = time.perf_counter()
    synth.genome(seed, n, 0, length)      # (the generator's library is built on first use: once, before the threads ask for it)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(seed, n, g, length), range(n)))
    ids = [eng.add_genome(s, o) for s, o in data]
    bases = sum(len(s) for s, _ in data)
    del data
    eng.upload()
    return ids, bases, round(time.perf_counter() - t0, 2)


def median_of(fn, repeats):
    """(what the last run returned, the median wall ms, every wall ms) of `repeats` runs after one warm-up."""
    fn()
    walls, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, round(statistics.median(walls), 3), [round(w, 3) for w in walls]


def counts_of(last):
    return {**{k: last[k] for k in ("n", "entries", "ignored", "representatives", "rounds", "launches")}, **{k: round(last[k], 3) for k in STAGES}}


def list_record(eng, name, a, b, w, n, score, repeats, want=None):
    def device():
        nodes = eng.screen_representatives(a, b, w, n=n, score=score)
        return nodes, eng.screen_representatives_last()
    (nodes, last), wall, walls = median_of(device, repeats)
    rec = {"list": name, "nodes": n, "entries": int(len(a)), "bytes_uploaded": int(len(a)) * (12 if w is not None else 8) + 8 * n, "bytes_read_back": 8 * n,
           "wall_ms_median": wall, "wall_ms_all": walls, "last": counts_of(last)}
    if want is not None:
        rec["equal_to_the_statement"] = bool((nodes[0] == want[0]).all() and (nodes[1] == want[1]).all())
    eng.screen_representatives_release()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_representatives_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "repeats": args.repeats, "timing": "median of the repeats after one warm-up",
              "not_measured": ["live-entry compaction between the batches (not implemented)", "several devices (MultiEngine.screen_dereplicate)",
                               f"collections beyond {args.genomes} genomes", "the dense path of screen_dereplicate", "run_dereplicate with exact=\"anim\""]}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def save():
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")

    with Engine(0) as eng:
        n = args.genomes
        ids, bases, prep = load(eng, SEED, n, args.length)
        opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
        print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)

        # ---- the index entry, the host's way, and the components -------------------------------------------------------------------------
        sc, wall, walls = median_of(lambda: eng.screen_dereplicate(ids, opt, path="index"), args.repeats)
        sizes = eng.screen_index(ids, KMER, args.scale)      # (the stages of a run of its own: screen_dereplicate releases what it leaves)
        need = screen.identity_thresholds(sizes, KMER, THRESHOLD, opt.min_shared)
        score = screen.score_keys(None, sizes)
        *_, n_pairs = eng.screen_index_representatives(need, score)
        last, ilast = eng.screen_representatives_last(), eng.screen_index_last()
        eng.screen_index_release()
        eng.screen_representatives_release()

        def host_way():
            sp = eng.screen_candidates(ids, opt, path="index")
            t0 = time.perf_counter()
            nodes = screen.representatives_of_pairs(sp.a, sp.b, sp.shared, n, screen.score_keys(None, sp.sizes))
            host_ms = (time.perf_counter() - t0) * 1e3
            return sp, screen.clusters_from_nodes(sp.labels, *nodes, screen.score_keys(None, sp.sizes)), host_ms
        (sp, hsc, host_ms), h_wall, h_walls = median_of(host_way, args.repeats)
        comps, c_wall, c_walls = median_of(lambda: eng.screen_components_of(ids, opt, path="index"), args.repeats)
        report["index_entry"] = {
            "genomes": n, "bases": bases, "options": dict(opt._asdict()), "kept_cells": int(n_pairs), "undirected_pairs_resident": int(n_pairs) // 2,
            "pair_list_bytes_on_device": 12 * (int(n_pairs) // 2), "representatives": int(len(sc.size)), "largest_cluster": int(sc.size.max()),
            "singletons": int((sc.size == 1).sum()),
            "device": {"wall_ms_median": wall, "wall_ms_all": walls, "bytes_read_back": 8 * n + 4 * n,
                       "stages": {"index_scan_ms": round(ilast["scan_ms"], 3), "index_sort_group_ms": round(ilast["sort_group_ms"], 3), **counts_of(last)}},
            "candidates_then_host_statement": {"wall_ms_median": h_wall, "wall_ms_all": h_walls, "host_statement_ms_last": round(host_ms, 3),
                                               "bytes_read_back": 12 * int(len(sp.a)) + 4 * n},
            "components_for_comparison": {"wall_ms_median": c_wall, "wall_ms_all": c_walls, "components": int(len(comps.size)), "largest_component": int(comps.size.max())},
            "equal": bool(all((getattr(sc, f) == getattr(hsc, f)).all() for f in screen.ScreenClusters._fields[1:])),
            "host_over_device": round(h_wall / wall, 3)}
        print(json.dumps(report["index_entry"]), flush=True)
        save()
        eng.clear_genomes()
        # ---- the list entry ----------------------------------------------------------------------------------------------------------------
        report["list_entry"] = [list_record(eng, f"kept pairs of {n} genomes (both directions)", sp.a, sp.b, sp.shared, n, score, args.repeats, (hsc.rep, hsc.via))]
        save()
        chain = np.arange(4095, dtype=np.int32)
        cscore = np.arange(4096, dtype=np.uint64)[::-1].copy()
        report["list_entry"].append(list_record(eng, "chain of 4096, scores falling along it", chain, chain + 1, None, 4096, cscore, args.repeats,
                                                screen.representatives_of_pairs(chain, chain + 1, None, 4096, cscore)))
        save()
        rng = np.random.default_rng(1)
        a = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        b = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        w = rng.integers(1, 5000, args.entries, dtype=np.uint32)
        rscore = rng.integers(0, 1 << 40, MAX_N).astype(np.uint64)
        report["list_entry"].append(list_record(eng, "random", a, b, w, MAX_N, rscore, args.repeats))
        save()
    print("wrote", out)


if __name__ == "__main__":
    main()
