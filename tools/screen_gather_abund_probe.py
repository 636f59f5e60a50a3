#!/usr/bin/env python3
"""Measure the gather's abundances on one MI355X.

  collection  the one of tools/screen_gather_probe.py: 32 768 + 1024 synthetic genomes, every 33rd held out, the other 32 768 indexed once.
  queries     the same mixtures — --members (4, 32, 256) held-out genomes in ONE multi-record genome, --queries (1, 64) such mixtures per
              call — with UNEQUAL copy numbers: member i of a mixture is joined (i mod 4) + 1 times.
  measured    per (members, queries), best of --repeats after one warm-up, wall milliseconds of: the plain gather count; the abundance
              count (Encode in place of Unique, the abundances beside the entries, the weights); the rounds; the abundance pass (rank
              table, attribute, sort, row statistics, read back).  Of the last run the HIP-event milliseconds of every stage
              (pg_screen_search_last, pg_screen_gather_last, pg_screen_gather_abund_last) and the bytes of the rank table.
  parent      --parent-tree DIR: a checkout of the PARENT commit with its library built.  A fresh child process imports pyani_amd from
              there and times ITS screen_gather_count on the same queries: what Encode and the weights cost is measured against the
              parent's code, not against the plain path of the code under test.  A second child does the same over THIS tree, plain
              count and abundance count: two processes that made the same calls in the same order, so that the ratios compare
              libraries and not what a process did before (the in-process counts above follow rounds and passes of the case before,
              whose allocations they inherit).  Without the option these records are left out.
  host        for one mixture (queries = 1): the same statistics in numpy — the attribution by rank over the winners' sets and the
              per-row sums, squares, extremes and medians — given the query's matched k-mers, their multiplicities and the rows; the
              sets come from the tests' numpy statement and are not timed.  For scale, and checked EQUAL to the device's integers.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_gather_abund_probe.json.

Usage: python tools/screen_gather_abund_probe.py [--members 4,32,256] [--queries 1,64] [--length 20000] [--scale 16] [--min-unique 20]
                                                 [--repeats 3] [--parent-tree DIR] [--out profiles/screen_gather_abund_probe.json]"""
import argparse
import json
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHILD = "--parent-child" in sys.argv      # the child imports the package of the tree named after the flag, and nothing of this one
sys.path.insert(0, sys.argv[sys.argv.index("--parent-child") + 1] if CHILD else str(ROOT))

import numpy as np      # noqa: E402

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402

KMER, SEED, N_DB, N_HELD = 16, 20261908, 32768, 1024


def join(genomes):
    seqs, off, base = [], [0], 0
    for s, o in genomes:
        seqs.append(np.asarray(s, dtype=np.uint8))
        off += [base + int(x) for x in o[1:]]
        base += int(o[-1])
    return np.concatenate(seqs), np.array(off, dtype=np.uint64)


def timed(fn, repeats):
    fn()      # warm-up: code objects, allocations
    walls, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, {"wall_ms_best": round(min(walls), 3), "wall_ms_all": [round(w, 3) for w in walls]}


def rounded(last, keys=None):
    return {k: (round(v, 3) if k.endswith("_ms") else v) for k, v in last.items() if keys is None or k in keys}


def collection(eng, args):
    """The index resident, the store cleared; (data, held, db)."""
    n = N_DB + N_HELD
    with ThreadPoolExecutor(16) as ex:
        data = list(ex.map(lambda g: synth.genome(SEED, n, g, args.length), range(n)))
    held = [g for g in range(n) if g % 33 == 32]
    held_set = set(held)
    db = [g for g in range(n) if g not in held_set]
    db_ids = [eng.add_genome(*data[g]) for g in db]
    eng.upload()
    eng.screen_search_index(db_ids, KMER, args.scale)
    eng.clear_genomes()
    return data, held, db


def mixtures(m, q, held):
    """q mixtures of m members: [[(genome, copies)]]"""
    return [[(held[(j * 17 + i * (N_HELD // m)) % N_HELD], i % 4 + 1) for i in range(m)] for j in range(q)]


def load_queries(eng, data, mixes):
    eng.clear_genomes()
    ids = [eng.add_genome(*join([data[g] for g, copies in mix for _ in range(copies)])) for mix in mixes]
    eng.upload()
    return ids


def cases(args):
    return [(m, q) for m in (int(x) for x in args.members.split(",") if x) for q in (int(x) for x in args.queries.split(",") if x)]


STAGES = ("query_keys", "lookups", "matched", "scan_ms", "sort_group_ms", "lookup_ms", "count_ms")


def parent_child(args):
    """In the child: the screen_gather_count of the tree it imported on the same queries — and the abundance count where that tree has
    one — as one JSON line on stdout."""
    import inspect
    out = {"library": _lib.load().pg_version().decode(), "cases": []}
    has_abundance = "abundance" in inspect.signature(Engine.screen_gather_count).parameters
    with Engine(0) as eng:
        data, held, _ = collection(eng, args)
        for m, q in cases(args):
            q_ids = load_queries(eng, data, mixtures(m, q, held))
            _, rec = timed(lambda: eng.screen_gather_count(q_ids), args.repeats)
            rec["count_stages"] = rounded(eng.screen_search_last(), STAGES)
            rec["expand_ms"] = round(eng.screen_gather_last()["expand_ms"], 3)
            rec = {"members": m, "queries": q, "count": rec}
            if has_abundance:
                _, rec["count_abund"] = timed(lambda: eng.screen_gather_count(q_ids, abundance=True), args.repeats)
                rec["count_abund"]["count_stages"] = rounded(eng.screen_search_last(), STAGES)
                rec["count_abund"]["expand_ms"] = round(eng.screen_gather_last()["expand_ms"], 3)
                rec["count_abund"]["weight_ms"] = round(eng.screen_gather_abundance_last()["weight_ms"], 3)
            out["cases"].append(rec)
        eng.screen_search_index_release()
    print("PARENT " + json.dumps(out), flush=True)


def run_child(tree, args):
    child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--parent-child", str(Path(tree).resolve()), "--members", args.members,
                            "--queries", args.queries, "--length", str(args.length), "--scale", str(args.scale), "--repeats", str(args.repeats)],
                           capture_output=True, text=True, timeout=600)
    lines = [x for x in child.stdout.splitlines() if x.startswith("PARENT ")]
    if child.returncode or not lines:
        raise SystemExit(f"the child over {tree} failed ({child.returncode}): {child.stderr[-2000:]}")
    got = json.loads(lines[-1][len("PARENT "):])
    return got["library"], {(c["members"], c["queries"]): c for c in got["cases"]}


def host_statistics(kmers, abund, winner_sets):
    """numpy: rank[x] = the first winner that holds x; per row the sorted multiplicities' sum, sum of squares, twice the median, min, max."""
    rank = np.full(len(kmers), len(winner_sets), dtype=np.int64)
    for t, s in enumerate(winner_sets):
        mine = np.isin(kmers, s, assume_unique=True) & (rank == len(winner_sets))
        rank[mine] = t
    keep = rank < len(winner_sets)
    order = np.lexsort((abund[keep], rank[keep]))
    r, a = rank[keep][order], abund[keep][order].astype(np.uint64)
    first = np.searchsorted(r, np.arange(len(winner_sets) + 1))
    m = np.diff(first)
    at = first[:-1]
    return (np.add.reduceat(a, at).tolist(), np.add.reduceat(a * a, at).tolist(), (a[at + (m - 1) // 2] + a[at + m // 2]).tolist(), a[at].tolist(),
            a[first[1:] - 1].tolist())


def host_route(data, db, mix, rows, stats, opt, repeats):
    from tests import screen_cases as scr
    occurrences = np.concatenate([scr.genome_occurrences(*data[g], opt.kmer, opt.scale) for g, copies in mix for _ in range(copies)])
    kmers, abund = np.unique(occurrences, return_counts=True)
    winner_sets = [scr.genome_set(*data[db[b]], opt.kmer, opt.scale) for b in rows[1].tolist()]
    got, rec = timed(lambda: host_statistics(kmers, abund, winner_sets), repeats)
    device = (stats[0].tolist(), stats[1][:, 0].tolist(), stats[2].tolist(), stats[3].tolist(), stats[4].tolist())      # (sums of squares below 2^64 here)
    rec["equal"] = bool(all(x == y for x, y in zip(got, device)) and not stats[1][:, 1].any())
    rec["query_kmers"] = int(len(kmers))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,32,256")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--min-unique", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_gather_abund_probe.json"))
    args = ap.parse_args()
    if CHILD:
        return parent_child(args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    opt = screen.GatherOptions(KMER, args.scale, args.min_unique, abundance=True)
    report = {"library": _lib.load().pg_version().decode(), "options": dict(opt._asdict()), "synthetic_length": args.length, "db_genomes": N_DB,
              "copies_of_member_i": "(i mod 4) + 1", "cases": []}
    parent, own = {}, {}
    if args.parent_tree:      # before this process opens the device, one after the other: one process on the GPU at a time
        report["parent_library"], parent = run_child(args.parent_tree, args)
        _, own = run_child(ROOT, args)
    with Engine(0) as eng:
        t0 = time.perf_counter()
        data, held, db = collection(eng, args)
        report["prepare_seconds"] = round(time.perf_counter() - t0, 2)
        for m, q in cases(args):
            mixes = mixtures(m, q, held)
            q_ids = load_queries(eng, data, mixes)
            rec = {"members": m, "queries": q}
            _, rec["count_plain"] = timed(lambda: eng.screen_gather_count(q_ids), args.repeats)
            rec["count_plain"]["count_stages"] = rounded(eng.screen_search_last(), STAGES)
            rec["count_plain"]["expand_ms"] = round(eng.screen_gather_last()["expand_ms"], 3)
            if (m, q) in parent:      # the like-for-like processes: the parent's count | this tree's plain and abundance counts
                rec["children"] = {"parent_count": parent[(m, q)]["count"], "count": own[(m, q)]["count"], "count_abund": own[(m, q)]["count_abund"]}
                rec["children"]["count_over_parent"] = round(own[(m, q)]["count"]["wall_ms_best"] / parent[(m, q)]["count"]["wall_ms_best"], 3)
                rec["children"]["count_abund_over_parent"] = round(own[(m, q)]["count_abund"]["wall_ms_best"] / parent[(m, q)]["count"]["wall_ms_best"], 3)
            (sizes, weight), rec["count_abund"] = timed(lambda: eng.screen_gather_count(q_ids, abundance=True), args.repeats)
            rec["count_abund"]["count_stages"] = rounded(eng.screen_search_last(), STAGES)
            rec["count_abund"]["expand_ms"] = round(eng.screen_gather_last()["expand_ms"], 3)
            rec["count_abund"]["weight_ms"] = round(eng.screen_gather_abundance_last()["weight_ms"], 3)
            rec["weight"] = int(weight.sum())
            rec["count_abund_over_plain"] = round(rec["count_abund"]["wall_ms_best"] / rec["count_plain"]["wall_ms_best"], 3)
            need = screen.gather_thresholds(sizes, opt.min_unique, opt.min_fraction)
            rows, rec["rounds"] = timed(lambda: eng.screen_gather_rows(need, opt.max_ranks), args.repeats)
            rec["rounds"]["last"] = rounded(eng.screen_gather_last())
            stats, rec["abundance_pass"] = timed(lambda: eng.screen_gather_abundance(), args.repeats)
            rec["abundance_pass"]["last"] = rounded(eng.screen_gather_abundance_last())
            rec["abundance_pass_over_rounds"] = round(rec["abundance_pass"]["wall_ms_best"] / rec["rounds"]["wall_ms_best"], 3)
            rec["rows"] = int(len(rows[0]))
            if q == 1:
                rec["host_numpy"] = host_route(data, db, mixes[0], rows, stats, opt, args.repeats)
                rec["host_over_abundance_pass"] = round(rec["host_numpy"]["wall_ms_best"] / rec["abundance_pass"]["wall_ms_best"], 3)
            report["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
        eng.screen_search_index_release()
    print("wrote", out)


if __name__ == "__main__":
    main()
