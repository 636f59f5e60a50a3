#!/usr/bin/env python3
"""Measure the components of the screen's kept pairs on one MI355X.  Best of --repeats after one warm-up; wall
milliseconds of the whole Python call, and the HIP-event milliseconds of pg_screen_components_last of the best run.

  list path    Engine.screen_components against scipy.sparse.csgraph.connected_components on the same list on the host, the COO build
               included: (a) the kept pairs of the 32 768-genome synthetic set of tools/screen_index_probe.py at identity 0.80, (b) a
               random list of 2^20 nodes and --entries entries (10^8: six upload chunks).  scipy runs --scipy-repeats times on (b).
               Beside them a star and a chain of 2^20 nodes each: every hook of the star contends on one tree, the chain is the deep one.
  index path   Engine.screen_components_of(path="index") against the way to the same table without this feature,
               Engine.screen_candidates(path="index") + the host statement screen.components_of_pairs, on the same 32 768 genomes; the
               bytes each reads back from the device.

No time is set in advance: what is measured is recorded, and what is not is listed under "not_measured".
Writes profiles/screen_components_probe.json.

Usage: python tools/screen_components_probe.py [--genomes 32768] [--length 20000] [--scale 16] [--entries 100000000] [--repeats 3]
                                               [--scipy-repeats 1] [--out profiles/screen_components_probe.json]"""
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

KMER, THRESHOLD, SEED = 16, 0.80, 20261908      # tools/screen_index_probe.py's: the same synthetic families of 25
MAX_N = 1 << 20


def load(eng, seed, n, length):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(seed, n, g, length), range(n)))
    ids = [eng.add_genome(s, o) for s, o in data]
    bases = sum(len(s) for s, _ in data)
    del data
    eng.upload()
    return ids, bases, round(time.perf_counter() - t0, 2)


def best_of(fn, repeats, warm=True):
    """(the result of the best run, its wall ms, every wall ms, what fn returned beside the result for the best run)."""
    if warm:
        fn()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        runs.append(((time.perf_counter() - t0) * 1e3, out))
    best = min(runs, key=lambda r: r[0])
    return best[1], round(best[0], 3), [round(r[0], 3) for r in runs]


def scipy_components(a, b, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    graph = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n))
    return connected_components(graph, directed=False)


def list_record(eng, name, a, b, s, n, repeats, scipy_repeats):
    def device():
        nodes = eng.screen_components(a, b, s, n=n)
        return nodes, eng.screen_components_last()
    (nodes, last), wall, walls = best_of(device, repeats)
    (count, label), s_wall, s_walls = best_of(lambda: scipy_components(a, b, n), scipy_repeats, warm=False)
    first = np.full(count, n, dtype=np.int64)
    np.minimum.at(first, label, np.arange(n))
    rec = {"list": name, "nodes": n, "entries": int(len(a)), "upload_chunks": -(-len(a) // (1 << 24)), "components": last["components"],
           "device": {"wall_ms_best": wall, "wall_ms_all": walls, "hook_ms": round(last["hook_ms"], 3), "flatten_ms": round(last["flatten_ms"], 3)},
           "scipy": {"wall_ms_best": s_wall, "wall_ms_all": s_walls, "repeats": scipy_repeats},
           "equal": bool(count == last["components"] and (first[label] == nodes[0]).all()),
           "scipy_over_device": round(s_wall / wall, 2)}
    eng.screen_components_release()
    print(json.dumps(rec), flush=True)
    return rec


def shape_record(eng, name, a, b, n, repeats):
    def device():
        nodes = eng.screen_components(a, b, None, n=n)
        return nodes, eng.screen_components_last()
    (nodes, last), wall, walls = best_of(device, repeats)
    rec = {"list": name, "nodes": n, "entries": int(len(a)), "components": last["components"], "wall_ms_best": wall, "wall_ms_all": walls,
           "hook_ms": round(last["hook_ms"], 3), "flatten_ms": round(last["flatten_ms"], 3), "all_rooted_at_0": bool((nodes[0] == 0).all())}
    eng.screen_components_release()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scipy-repeats", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_components_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "repeats": args.repeats,
              "not_measured": ["several devices (MultiEngine.screen_components_of)", f"collections beyond {args.genomes} genomes",
                               "more than one upload chunk on a list from a screen (only the random list has six)",
                               "the dense path of screen_components_of"]}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def save():
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")

    with Engine(0) as eng:
        # ---- the index path, and the kept pairs of the same set for the list path ----------------------------------------------------
        n = args.genomes
        ids, bases, prep = load(eng, SEED, n, args.length)
        opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
        print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)

        def device():
            sc = eng.screen_components_of(ids, opt, path="index")
            return sc

        def parent_way():
            sp = eng.screen_candidates(ids, opt, path="index")
            t0 = time.perf_counter()
            nodes = screen.components_of_pairs(sp.a, sp.b, sp.shared, n)
            host_ms = (time.perf_counter() - t0) * 1e3
            return sp, screen.components_from_nodes(sp.labels, *nodes), host_ms
        sc, wall, walls = best_of(device, args.repeats)
        # (the stage milliseconds of a run of its own: screen_components_of releases what it leaves)
        sizes = eng.screen_index(ids, KMER, args.scale)
        need = screen.identity_thresholds(sizes, KMER, THRESHOLD, opt.min_shared)
        *_, n_pairs = eng.screen_index_components(need)
        last, ilast = eng.screen_components_last(), eng.screen_index_last()
        eng.screen_index_release()
        eng.screen_components_release()
        (sp, psc, host_ms), p_wall, p_walls = best_of(parent_way, args.repeats)
        report["index_path"] = {
            "genomes": n, "bases": bases, "options": dict(opt._asdict()), "kept_pairs": int(n_pairs), "components": int(len(sc.size)),
            "largest_component": int(sc.size.max()), "singletons": int((sc.size == 1).sum()),
            "device": {"wall_ms_best": wall, "wall_ms_all": walls, "bytes_read_back": 24 * n,
                       "stages": {"index_scan_ms": round(ilast["scan_ms"], 3), "index_sort_group_ms": round(ilast["sort_group_ms"], 3),
                                  "band_count_select_ms": round(last["select_ms"], 3), "hook_accumulate_ms": round(last["hook_ms"], 3),
                                  "flatten_ms": round(last["flatten_ms"], 3)}},
            "candidates_then_host": {"wall_ms_best": p_wall, "wall_ms_all": p_walls, "host_statement_ms": round(host_ms, 3),
                                     "bytes_read_back": 12 * int(len(sp.a)) + 4 * n},
            "equal": bool(all((getattr(sc, f) == getattr(psc, f)).all() for f in screen.ScreenComponents._fields[1:])),
            "candidates_then_host_over_device": round(p_wall / wall, 3)}
        print(json.dumps(report["index_path"]), flush=True)
        save()
        eng.clear_genomes()
        report["list_path"] = [list_record(eng, f"kept pairs of {n} genomes", sp.a, sp.b, sp.shared, n, args.repeats, args.repeats)]
        save()
        # ---- shapes: contention and depth ------------------------------------------------------------------------------------------------
        leaves = np.arange(MAX_N - 1, dtype=np.int32)
        report["shapes"] = [shape_record(eng, "star, hub 2^20 - 1", np.full(MAX_N - 1, MAX_N - 1, np.int32), leaves, MAX_N, args.repeats),
                            shape_record(eng, "chain, ascending", leaves, leaves + 1, MAX_N, args.repeats),
                            shape_record(eng, "chain, descending", leaves[::-1].copy(), leaves[::-1] + 1, MAX_N, args.repeats)]
        save()
        # ---- the random list -----------------------------------------------------------------------------------------------------------------
        rng = np.random.default_rng(1)
        a = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        b = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
        s = rng.integers(1, 5000, args.entries, dtype=np.uint32)
        report["list_path"].append(list_record(eng, "random", a, b, s, MAX_N, args.repeats, args.scipy_repeats))
        save()
    print("wrote", out)


if __name__ == "__main__":
    main()
