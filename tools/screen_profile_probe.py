#!/usr/bin/env python3
"""Measure the profile of a partition over the resident search index on one MI355X.  Every device call runs --repeats
times after one warm-up; the MEDIAN wall milliseconds of the whole Python call (checks, upload of the partition, kernels, read-back of
the thirteen arrays and the marker list) are reported beside every run's, with the HIP-event milliseconds and counts of
pg_screen_search_profile_last of the last run.  The baseline is the route that existed before: Engine.screen_search_index_export, then
the numpy statement screen.profile_of_index on the host, timed as one call --repeats times without a warm-up (numpy has nothing to
warm), with the bytes it reads back.  EVERY device run is compared with the statement for equality and the comparison recorded.

  set      the 32 768-genome synthetic set of the other screen probes, indexed at scale 16, under its greedy representatives, under its
           components and with every genome its own cluster.
  tiers    the same set under its greedy representatives over the settable tier limits: the table the defaults are chosen from.
  sorted   a hand-made worst case for the sorted tier: a few k-mers held by all 2^20 genomes (one cluster; 2^19 pairs).

Three runs show a median and its spread on an otherwise shared host; they cannot resolve differences of a few per cent.  No ratio is
set in advance: what is measured is recorded, a workload the device loses included, and what is not is listed under "not_measured".
Writes profiles/screen_profile_probe.json.

Usage: python tools/screen_profile_probe.py [--sections set,tiers,sorted] [--genomes 32768] [--length 20000] [--scale 16] [--repeats 3]
                                            [--out profiles/screen_profile_probe.json]"""
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
STAGES = ("relabel_ms", "lane_ms", "wave_ms", "sorted_ms", "marker_ms")
COUNTS = ("n", "clusters", "kmers", "entries", "cells", "lane_kmers", "wave_kmers", "sorted_kmers", "sorted_batches", "markers")
LANE_LIMITS, WAVE_LIMITS = (0, 1, 2, 4, 8), (8, 16, 32, 64)


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


def arrays_of(p):
    return list(p.genome_arrays()) + list(p.cluster_arrays()) + [p.spectrum] + list(p.marker_arrays())


def equal(p, want):
    genomes, clusters, spectrum, _, markers = want
    flat = list(genomes) + list(clusters) + [spectrum] + list(markers)
    return bool(all(g.shape == w.shape and (g == w).all() for g, w in zip(arrays_of(p), flat)))


def counts_of(last):
    return {**{k: last[k] for k in COUNTS}, **{k: round(last[k], 3) for k in STAGES}}


def sampled_kmers(count, k, scale):
    """`count` distinct sampled k-mers, ascending (one slice holds them in this order)."""
    out, x = [], 0
    while len(out) < count:
        block = np.arange(x, x + 4096, dtype=np.uint32)
        out += block[screen.kmer_sampled(block, scale)].tolist()
        x += 4096
    return np.array(out[:count], dtype=np.uint32)


def record(eng, name, label, repeats, host_runs=None):
    """One workload over the resident index: the device's profile against export + the host statement."""
    n = len(label)
    need = screen.profile_thresholds(np.bincount(label, minlength=n))

    def host_way():
        shape, (kmer, start, member, _, _) = eng.screen_search_index_export()
        t0 = time.perf_counter()
        out = screen.profile_of_index(kmer, start, member, n, label, *need, 2)
        return out, shape, (time.perf_counter() - t0) * 1e3
    hosts, h_wall, h_walls = timed(host_way, host_runs or repeats, warm_up=False)
    want, shape = hosts[0][0], hosts[0][1]

    def device():
        p = eng.screen_search_profile(label)
        return p, eng.screen_search_profile_last()
    outs, wall, walls = timed(device, repeats, warm_up=True)
    p, last = outs[-1]
    d, e = shape[3], shape[4]
    rec = {"partition": name, "genomes": n, "kmers": d, "entries": e, "clusters": int(len(p.naming())), "largest_cluster": int(p.size.max()),
           "markers_listed": int(len(p.marker_kmer)), "cells": last["cells"],
           "device": {"wall_ms_median": wall, "wall_ms_all": walls, "bytes_uploaded": 12 * n,
                      "bytes_read_back": 4 * 5 * n + 4 * n + 8 * 6 * n + 8 * n + 12 * int(len(p.marker_kmer)), "last": counts_of(last)},
           "export_then_host_statement": {"wall_ms_median": h_wall, "wall_ms_all": h_walls, "host_statement_ms_all": [round(h[2], 3) for h in hosts],
                                          "bytes_read_back": 12 * d + 4 * e + 8 + 8 * (shape[5] + 1) + 4 * 4096},
           "equal_to_the_statement_every_run": [equal(q, want) for q, _ in outs], "host_over_device": round(h_wall / wall, 3)}
    print(json.dumps(rec), flush=True)
    return rec, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="set,tiers,sorted")
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_profile_probe.json"))
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    report = json.loads(out.read_text()) if out.exists() else {}
    report.update({"library": _lib.load().pg_version().decode(), "kmer": KMER, "scale": args.scale, "min_identity": THRESHOLD, "repeats": args.repeats,
                   "timing": "device: median of the repeats after one warm-up; export + host statement: median of the repeats, no warm-up",
                   "not_measured": ["several devices (a dealt index is not profiled)", f"collections beyond {args.genomes} genomes", "run_screen_profile (the driver)",
                                    "batch_keys below the default on the set (its sorted tier fits one batch)", "kernel times by rocprofv3 (the stages are HIP events)"]})

    def save():
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")

    with Engine(0) as eng:
        if sections & {"set", "tiers"}:
            n = args.genomes
            ids, bases, prep = load(eng, SEED, n, args.length)
            opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
            print("resident:", n, "genomes,", bases, "bases,", prep, "s", flush=True)
            rep = eng.screen_dereplicate(ids, opt, path="index").rep
            root = eng.screen_components_of(ids, opt, path="index").root
            eng.screen_search_index(ids, KMER, args.scale)
            eng.clear_genomes()      # (the index and the profile read nothing of the store)
            report["set"] = {"genomes": n, "bases": bases, "options": dict(opt._asdict()), "index": {k: eng.screen_search_last()[k] for k in ("kmers", "entries", "slices", "index_bytes")}}
        if "set" in sections:
            report["set"]["workloads"] = {}
            for name, label in (("greedy representatives", rep), ("components", root), ("every genome its own cluster", np.arange(n, dtype=np.int32))):
                report["set"]["workloads"][name], _ = record(eng, name, np.ascontiguousarray(label, dtype=np.int32), args.repeats)
                save()
        if "tiers" in sections:
            label = np.ascontiguousarray(rep, dtype=np.int32)
            need = screen.profile_thresholds(np.bincount(label, minlength=n))
            _, (kmer, start, member, _, _) = eng.screen_search_index_export()
            want = screen.profile_of_index(kmer, start, member, n, label, *need, 2)
            del kmer, start, member
            rows = []
            for lane, wave in [(0, 0)] + [(a, b) for a in LANE_LIMITS for b in WAVE_LIMITS if a <= b]:
                eng.screen_search_profile_set(lane, wave, 0)

                def device():
                    p = eng.screen_search_profile(label)
                    return p, eng.screen_search_profile_last()
                outs, wall, walls = timed(device, args.repeats, warm_up=True)
                rows.append({"lane_limit": lane, "wave_limit": wave, "wall_ms_median": wall, "wall_ms_all": walls, "last": counts_of(outs[-1][1]),
                             "equal_to_the_statement_every_run": [equal(q, want) for q, _ in outs]})
                print(json.dumps(rows[-1]), flush=True)
            eng.screen_search_profile_set()
            best = min(rows, key=lambda r: r["wall_ms_median"])
            report["tiers"] = {"partition": "greedy representatives", "genomes": n, "rows": rows, "fastest": {"lane_limit": best["lane_limit"], "wave_limit": best["wave_limit"],
                                                                                                              "wall_ms_median": best["wall_ms_median"]}}
            save()
        eng.screen_search_profile_release()
        eng.screen_search_index_release()
        if "sorted" in sections:
            few, n = 4, MAX_N
            kmer = sampled_kmers(few, KMER, args.scale)
            start = (np.arange(few + 1, dtype=np.uint64) * np.uint64(n))
            member = np.tile(np.arange(n, dtype=np.uint32), few)
            eng.screen_search_index_import((n, KMER, args.scale, few, few * n, 1, few * n), (kmer, start, member, np.array([0, few], dtype=np.uint64), np.zeros(4096, dtype=np.uint32)))
            report["sorted"] = {"genomes": n, "kmers_held_by_all": few, "workloads": {}}
            for name, label in (("one cluster", np.zeros(n, dtype=np.int32)), ("2^19 pairs", np.arange(n, dtype=np.int32) & ~np.int32(1))):
                report["sorted"]["workloads"][name], _ = record(eng, name, label, args.repeats)
                save()
            eng.screen_search_profile_release()
            eng.screen_search_index_release()
    print("wrote", out)


if __name__ == "__main__":
    main()
