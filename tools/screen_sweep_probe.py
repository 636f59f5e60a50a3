#!/usr/bin/env python3
"""Measure the sweep of the components over a ladder of thresholds on one MI355X, against the route that existed
before it: one components call per step.  Every timed call runs --repeats times after one warm-up; the BEST wall milliseconds of the
whole Python call are reported beside every run's, and the HIP-event milliseconds and counts of pg_screen_sweep_last of a run of its own.
Where a per-step route would take minutes it runs ONCE, without a warm-up, and the record says so ("runs": 1).

  index form   Engine.screen_sweep_of(path="index") on the 32 768-genome synthetic set of tools/screen_index_probe.py with ladders of
               8, 64 and 512 identities between 0.80 and 0.995 — the index built, the bands selected once by the lowest step, the
               levels found on the device, one sort, one descending pass — against
                 per_step_of     one Engine.screen_components_of(path="index") per step: what a caller had (the index rebuilt per call), and
                 per_step_lean   the index built ONCE and one Engine.screen_index_components per step: the least the old calls allow.
  list form    Engine.screen_sweep on the pairs kept at 0.80 with the host's levels, against one Engine.screen_components per step over
               the entries present there (the list sorted by level once on the host, so that a step's entries are a prefix: no host
               work per step is timed).
  random       --entries (10^8) random entries over 2^20 nodes with 64 levels, against 64 list calls.
  bad case     2^20 nodes, 4 x 10^6 random entries, every level of the ladder held by some entry: a census at every step; with 512
               and with 4096 steps.

The results of the two routes are compared in every run ("equal").  "Touched components only" as a census was NOT tried: every census
visits all n nodes.  No time is set in advance: what is measured is recorded.  Writes profiles/screen_sweep_probe.json.

Usage: python tools/screen_sweep_probe.py [--genomes 32768] [--length 20000] [--scale 16] [--entries 100000000] [--repeats 3]
                                          [--out profiles/screen_sweep_probe.json]"""
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

KMER, SEED = 16, 20261908      # tools/screen_index_probe.py's: the same synthetic families of 25
LOW, HIGH = 0.80, 0.995
MAX_N = 1 << 20
STAGES = ("select_ms", "sort_ms", "hook_ms", "census_ms")
ONCE_ABOVE_S = 60.0      # a per-step route expected to take longer than this runs once


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


def best_of(fn, repeats, warm=True):
    """(what the last run returned, the best wall ms, every wall ms) of `repeats` runs after one warm-up."""
    if warm:
        fn()
    walls, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, round(min(walls), 3), [round(w, 3) for w in walls]


def timed(rec, name, fn, repeats, expect_s):
    once = expect_s > ONCE_ABOVE_S
    out, best, walls = best_of(fn, 1 if once else repeats, warm=not once)
    rec[name] = {"wall_ms_best": best, "wall_ms_all": walls, "runs": len(walls), "warm_up": not once}
    return out


def figures(root, entries):
    size = np.bincount(root, minlength=len(root)).astype(np.uint64)
    size = size[size > 0]
    return int(entries.sum()), len(size), int((size == 1).sum()), int(size.max()), int((size * (size - np.uint64(1))).sum())


def same(arrays, rows, steps=None):
    """The sweep's five arrays against the per-step route's figures at `steps` (all when None)."""
    steps = range(len(rows)) if steps is None else steps
    return bool(all(tuple(int(x[s]) for x in arrays[:5]) == tuple(rows[s]) for s in steps))


def counts_of(last):
    return {**{k: last[k] for k in ("n", "steps", "entries", "ignored", "level0", "buckets")}, **{k: round(last[k], 3) for k in STAGES}}


def by_level(a, b, w, level):
    """The list sorted by level, descending (stable), and for every step the number of entries present: step s is the prefix [:present[s]]."""
    order = np.argsort(-level.astype(np.int32), kind="stable")
    steps = int(level.max()) if len(level) else 1
    hist = np.bincount(level, minlength=steps + 1)
    return a[order], b[order], None if w is None else w[order], level[order], [int(hist[s + 1:].sum()) for s in range(steps)]


def list_record(eng, name, a, b, w, level, n, steps, repeats, per_step_s, compare=None):
    """One list workload: the sweep, and one components call per step over the entries present there."""
    rec = {"list": name, "nodes": n, "entries": int(len(a)), "steps": steps}

    def sweep():
        return eng.screen_sweep(a, b, w, level, n=n, steps=steps)
    arrays = timed(rec, "sweep", sweep, repeats, 0.0)
    rec["sweep"]["last"] = counts_of(eng.screen_sweep_last())
    eng.screen_sweep_release()
    sa, sb, sw, _, present = by_level(a, b, w, level)
    present += [0] * (steps - len(present))
    compare = range(steps) if compare is None else compare

    def per_step():
        rows = {}
        for s in range(steps):
            root, entries, _ = eng.screen_components(sa[:present[s]], sb[:present[s]], None if sw is None else sw[:present[s]], n=n)
            if s in compare:
                rows[s] = figures(root, entries)
            else:
                rows[s] = (None, eng.screen_components_last()["components"])
        return rows
    rows = timed(rec, "per_step_list_calls", per_step, repeats, per_step_s)
    eng.screen_components_release()
    rec["equal"] = same(arrays, rows, compare) and all(int(arrays[1][s]) == rows[s][1] for s in range(steps))
    rec["figures_compared_at_steps"] = len(list(compare))
    rec["per_step_over_sweep"] = round(rec["per_step_list_calls"]["wall_ms_best"] / rec["sweep"]["wall_ms_best"], 3)
    rec["complete_steps"] = int((arrays[4] == arrays[0]).sum())
    rec["components_first_last"] = [int(arrays[1][0]), int(arrays[1][-1])]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ladders", type=int, nargs="*", default=[8, 64, 512])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_sweep_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "ladder": [LOW, HIGH], "repeats": args.repeats,
              "timing": "best of the repeats after one warm-up, the whole Python call; runs == 1: once, no warm-up",
              "not_measured": ["a census of the touched components only (not implemented: every census visits all n nodes)", "several devices (MultiEngine has no sweep)",
                               f"collections beyond {args.genomes} genomes", "the dense path of screen_sweep_of", "an exact=\"anim\" driver over levels_of_values"]}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def save():
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")

    with Engine(0) as eng:
        n = args.genomes
        ids, bases, prep = load(eng, SEED, n, args.length)
        print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)
        one_call_s = None
        report["index_form"], report["list_form"] = [], []
        for S in args.ladders:
            ladder = np.linspace(LOW, HIGH, S)
            opt = screen.ScreenOptions(float(ladder[0]), KMER, args.scale)
            rec = {"genomes": n, "bases": bases, "steps": S, "options": dict(opt._asdict())}
            sw = timed(rec, "sweep", lambda: eng.screen_sweep_of(ids, opt, ladder, path="index"), args.repeats, 0.0)
            sizes = eng.screen_index(ids, KMER, args.scale)      # (the stages of a run of its own: screen_sweep_of releases what it leaves)
            t0 = time.perf_counter()
            need = screen.sweep_thresholds(sizes, KMER, ladder, opt.min_shared)
            rec["host_table_ms"] = round((time.perf_counter() - t0) * 1e3, 3)      # (inside the sweep's wall time; the per-step routes pay one row per call)
            *arrays, n_pairs = eng.screen_index_sweep(need)
            ilast = eng.screen_index_last()
            rec["sweep"]["stages"] = {"index_scan_ms": round(ilast["scan_ms"], 3), "index_sort_group_ms": round(ilast["sort_group_ms"], 3), **counts_of(eng.screen_sweep_last())}
            rec["kept_cells_at_the_lowest_step"] = int(n_pairs)
            rec["need_table_bytes"] = int(need.nbytes)
            eng.screen_index_release()
            eng.screen_sweep_release()

            def lean():
                eng.screen_index(ids, KMER, args.scale)
                rows = []
                for s in range(S):
                    root, entries, _, _ = eng.screen_index_components(need[s])
                    rows.append(figures(root, entries))
                eng.screen_index_release()
                eng.screen_components_release()
                return rows
            rows = timed(rec, "per_step_lean", lean, args.repeats, 0.0 if one_call_s is None else S * one_call_s * 0.25)

            def of():
                return [eng.screen_components_of(ids, screen.ScreenOptions(float(t), KMER, args.scale), path="index") for t in ladder]
            comps = timed(rec, "per_step_of", of, args.repeats, 0.0 if one_call_s is None else S * one_call_s)
            one_call_s = rec["per_step_of"]["wall_ms_best"] / 1e3 / S
            rec["equal"] = bool(same(arrays, rows) and same([sw.entries, sw.components, sw.singletons, sw.largest, sw.pair_slots], rows) and
                                all(len(c.size) == rows[s][1] and int(c.size.max()) == rows[s][3] for s, c in enumerate(comps)))
            rec["per_step_of_over_sweep"] = round(rec["per_step_of"]["wall_ms_best"] / rec["sweep"]["wall_ms_best"], 3)
            rec["per_step_lean_over_sweep"] = round(rec["per_step_lean"]["wall_ms_best"] / rec["sweep"]["wall_ms_best"], 3)
            rec["complete_steps"] = int(sw.complete.sum())
            rec["components_first_last"] = [int(sw.components[0]), int(sw.components[-1])]
            report["index_form"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
        sp = eng.screen_candidates(ids, screen.ScreenOptions(LOW, KMER, args.scale), path="index")
        eng.clear_genomes()
        for S in args.ladders:
            ladder = np.linspace(LOW, HIGH, S)
            t0 = time.perf_counter()
            level = screen.sweep_levels(sp.a, sp.b, sp.shared, screen.sweep_thresholds(sp.sizes, KMER, ladder, sp.options.min_shared))
            host_ms = (time.perf_counter() - t0) * 1e3
            rec = list_record(eng, f"pairs of {n} genomes kept at {LOW} (both directions), {S} steps", sp.a, sp.b, sp.shared, level, n, S, args.repeats, 0.0)
            rec["host_levels_ms"] = round(host_ms, 3)
            report["list_form"].append(rec)
            save()
        del sp
        # ---- random entries over 2^20 nodes ---------------------------------------------------------------------------------------------------
        rng = np.random.default_rng(1)
        a = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        b = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        w = rng.integers(1, 5000, args.entries, dtype=np.uint32)
        level = rng.integers(1, 65, args.entries).astype(np.uint16)
        report["random"] = list_record(eng, "random, 64 levels", a, b, w, level, MAX_N, 64, args.repeats, 0.0)
        save()
        del a, b, w, level
        # ---- the bad case: a census at every step -----------------------------------------------------------------------------------------------
        report["bad_case"] = []
        m = 4_000_000
        a = rng.integers(0, MAX_N, m, dtype=np.int32)
        b = rng.integers(0, MAX_N, m, dtype=np.int32)
        for S, expect_s in ((512, 0.0), (4096, 4 * ONCE_ABOVE_S)):
            level = (1 + np.arange(m) % S).astype(np.uint16)      # every level 1 ... S is held
            compare = sorted(set(np.linspace(0, S - 1, 16).astype(int).tolist()))
            report["bad_case"].append(list_record(eng, f"random, every one of {S} buckets non-empty", a, b, None, level, MAX_N, S, args.repeats, expect_s, compare))
            save()
    print("wrote", out)


if __name__ == "__main__":
    main()
