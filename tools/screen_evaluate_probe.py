#!/usr/bin/env python3
"""Measure the evaluation of a partition of the screen's kept pairs on one MI355X, on the workloads of
tools/screen_representatives_probe.py, so that the rows of the two files sit side by side.  Every device call runs --repeats times after
one warm-up; the MEDIAN wall milliseconds of the whole Python call (upload, kernels, read-back of the fourteen arrays) are reported
beside every run's, with the HIP-event milliseconds and counts of pg_screen_evaluate_last of the last run.  The host's way is the numpy
statement screen.evaluate_of_pairs, timed --repeats times without a warm-up (numpy has nothing to warm) — ONCE for a list beyond
2 x 10^7 entries, where one run takes minutes; the record's wall_ms_all shows which; EVERY device run is compared with the statement
for equality and the comparison recorded.

  index    Engine.screen_evaluate_of(path="index") on the 32 768-genome synthetic set at identity 0.80, the partition = the greedy
           representatives — the index built, all bands selected, the undirected kept pairs appended on the device, pair and node passes
           — against Engine.screen_candidates(path="index") + the host statement; the bytes read back on either way.
  list     Engine.screen_evaluate on the kept pairs of that set (both directions, as the selection returns them) against the statement.
  random   --entries entries (10^8) over 2^20 nodes under a random partition of about 2^16 clusters.
  dense    the hub star (2^20 - 1 leaves, one cluster) and one cluster of 8192 nodes as a clique (3.4 x 10^7 pairs).

Three runs show a median and its spread on an otherwise shared host; they cannot resolve differences of a few per cent.  No time is
set in advance: what is measured is recorded, and what is not is listed under "not_measured".  Sections named in --sections are run and
merged into the file already there.  Writes profiles/screen_evaluate_probe.json.

Usage: python tools/screen_evaluate_probe.py [--sections index,list,random,dense] [--genomes 32768] [--length 20000] [--scale 16]
                                             [--entries 100000000] [--repeats 3] [--out profiles/screen_evaluate_probe.json]"""
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
HOST_ONCE_ABOVE = 20_000_000      # entries: the host statement takes minutes beyond
STAGES = ("select_ms", "sort_ms", "pair_ms", "node_ms")
RESULT_BYTES_PER_NODE = 4 * 5 + 8 + 4 + 4 * 3 + 8 * 2 + 4 * 2      # the seven node arrays and the seven cluster arrays


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


def timed(fn, repeats, warm_up):
    """(what every run returned, the median wall ms, every wall ms) of `repeats` runs, after one warm-up if asked."""
    if warm_up:
        fn()
    walls, outs = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        outs.append(fn())
        walls.append((time.perf_counter() - t0) * 1e3)
    return outs, round(statistics.median(walls), 3), [round(w, 3) for w in walls]


def equal(got, want):
    return bool(all((g == w).all() for half_g, half_w in zip(got, want) for g, w in zip(half_g, half_w)))


def counts_of(last):
    return {**{k: last[k] for k in ("n", "entries", "ignored", "pairs", "inside", "clusters")}, **{k: round(last[k], 3) for k in STAGES}}


def random_partition(rng, n, clusters):
    group = rng.integers(0, clusters, n)
    first = np.full(clusters, n, dtype=np.int64)
    np.minimum.at(first, group, np.arange(n))
    return first[group].astype(np.int32)


def list_record(eng, name, a, b, w, n, label, score, repeats):
    host_runs = repeats if len(a) <= HOST_ONCE_ABOVE else 1      # (minutes a run beyond: one run, said so in the record)
    wants, h_wall, h_walls = timed(lambda: screen.evaluate_of_pairs(a, b, w, n, label, score), host_runs, warm_up=False)

    def device():
        out = eng.screen_evaluate(a, b, w, n=n, label=label, score=score)
        return out, eng.screen_evaluate_last()
    outs, wall, walls = timed(device, repeats, warm_up=True)
    rec = {"list": name, "nodes": n, "entries": int(len(a)), "bytes_uploaded": int(len(a)) * (12 if w is not None else 8) + 12 * n,
           "bytes_read_back": RESULT_BYTES_PER_NODE * n, "device": {"wall_ms_median": wall, "wall_ms_all": walls, "last": counts_of(outs[-1][1])},
           "host_statement": {"wall_ms_median": h_wall, "wall_ms_all": h_walls},
           "equal_to_the_statement_every_run": [equal(got, wants[0]) for got, _ in outs], "host_over_device": round(h_wall / wall, 3)}
    eng.screen_evaluate_release()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="index,list,random,dense")
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_evaluate_probe.json"))
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    report = json.loads(out.read_text()) if out.exists() else {}
    report.update({"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "repeats": args.repeats,
                   "timing": "device: median of the repeats after one warm-up; host statement: median of the repeats, no warm-up",
                   "not_measured": ["several devices (the evaluation runs on the first engine)", f"collections beyond {args.genomes} genomes",
                                    "the dense path of screen_evaluate_of", "run_dereplicate(evaluate=True)", "kernel times by rocprofv3 (the stages are HIP events)"]})
    report.setdefault("list_entry", {})

    def save():
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")

    with Engine(0) as eng:
        if sections & {"index", "list"}:
            n = args.genomes
            ids, bases, prep = load(eng, SEED, n, args.length)
            opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
            print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)
            label = eng.screen_dereplicate(ids, opt, path="index").rep
            sp = eng.screen_candidates(ids, opt, path="index")
            score = screen.score_keys(None, sp.sizes)
        if "index" in sections:
            outs, wall, walls = timed(lambda: eng.screen_evaluate_of(ids, opt, label, path="index"), args.repeats, warm_up=True)
            sizes = eng.screen_index(ids, KMER, args.scale)      # (the stages of a run of its own: screen_evaluate_of releases what it leaves)
            need = screen.identity_thresholds(sizes, KMER, THRESHOLD, opt.min_shared)
            *_, n_pairs = eng.screen_index_evaluate(need, label, score)
            last, ilast = eng.screen_evaluate_last(), eng.screen_index_last()
            eng.screen_index_release()
            eng.screen_evaluate_release()

            def host_way():
                kept = eng.screen_candidates(ids, opt, path="index")
                t0 = time.perf_counter()
                halves = screen.evaluate_of_pairs(kept.a, kept.b, kept.shared, n, label, screen.score_keys(None, kept.sizes))
                return kept, halves, (time.perf_counter() - t0) * 1e3
            hosts, h_wall, h_walls = timed(host_way, args.repeats, warm_up=True)
            want = hosts[-1][1]
            ev = outs[-1]
            report["index_entry"] = {
                "genomes": n, "bases": bases, "options": dict(opt._asdict()), "kept_cells": int(n_pairs), "undirected_pairs_resident": int(n_pairs) // 2,
                "pair_list_bytes_on_device": 12 * (int(n_pairs) // 2), "clusters": int(len(ev.naming())), "largest_cluster": int(ev.size.max()),
                "complete_clusters": int(ev.complete().sum()), "clusters_with_a_near_cluster": int(len(ev.proximity(0))),
                "device": {"wall_ms_median": wall, "wall_ms_all": walls, "bytes_read_back": RESULT_BYTES_PER_NODE * n + 4 * n,
                           "stages": {"index_scan_ms": round(ilast["scan_ms"], 3), "index_sort_group_ms": round(ilast["sort_group_ms"], 3), **counts_of(last)}},
                "candidates_then_host_statement": {"wall_ms_median": h_wall, "wall_ms_all": h_walls, "host_statement_ms_all": [round(h[2], 3) for h in hosts],
                                                   "bytes_read_back": 12 * int(len(hosts[-1][0].a)) + 4 * n},
                "equal_every_run": [equal((e.node_arrays(), e.cluster_arrays()), want) for e in outs],
                "host_over_device": round(h_wall / wall, 3)}
            print(json.dumps(report["index_entry"]), flush=True)
            save()
        eng.clear_genomes()
        if "list" in sections:
            report["list_entry"]["kept_pairs"] = list_record(eng, f"kept pairs of {n} genomes (both directions)", sp.a, sp.b, sp.shared, n, label, score, args.repeats)
            save()
        rng = np.random.default_rng(1)
        if "random" in sections:
            a = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
            b = rng.integers(0, MAX_N, args.entries, dtype=np.int32)
            w = rng.integers(1, 5000, args.entries, dtype=np.uint32)
            rscore = rng.integers(0, 1 << 40, MAX_N).astype(np.uint64)
            report["list_entry"]["random"] = list_record(eng, "random entries, a random partition of about 2^16 clusters", a, b, w, MAX_N,
                                                         random_partition(rng, MAX_N, 1 << 16), rscore, args.repeats)
            del a, b, w
            save()
        if "dense" in sections:
            leaves = np.arange(1, MAX_N, dtype=np.int32)
            report["list_entry"]["hub_star"] = list_record(eng, "hub star: node 0 and 2^20 - 1 leaves in one cluster", np.zeros(MAX_N - 1, np.int32), leaves,
                                                           rng.integers(1, 5000, MAX_N - 1, dtype=np.uint32), MAX_N, np.zeros(MAX_N, np.int32),
                                                           np.arange(MAX_N, dtype=np.uint64), args.repeats)
            save()
            i, j = np.triu_indices(8192, 1)
            report["list_entry"]["clique"] = list_record(eng, "one cluster of 8192 nodes as a clique", i.astype(np.int32), j.astype(np.int32),
                                                         rng.integers(1, 5000, len(i), dtype=np.uint32), 8192, np.zeros(8192, np.int32),
                                                         np.arange(8192, dtype=np.uint64), args.repeats)
            save()
    print("wrote", out)


if __name__ == "__main__":
    main()
